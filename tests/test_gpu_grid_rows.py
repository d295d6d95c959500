"""Entries whose kernels take a job per grid row, past the 65 535 rows a grid has (`launch_rows`, csrc/common.hpp): the second launch
must start at job 65 535 with every per-job pointer moved on, and with every pointer that is indexed some other way left where it is.
tests/test_gpu_hsva.py has this for spng_hsva_batch (test_a_large_batch_crosses_the_grid_limit); here is every other entry that
splits a launch, one call of N = 65 537 jobs each through the C ABI: jobs that differ from their neighbours, slices of one or two
device tensors, every output and every result row compared with the suite's plain restatements, guard bytes between and behind the
outputs, and -- where an entry reports a failure per job -- failing jobs planted on both sides of the limit.

    launch site (csrc)                                        crossed by
    alpha, luminance                                          test_alpha_and_luminance_batches_cross_the_grid_limit
    text_count, text_write (text.hip)                         test_text_batch_crosses_the_grid_limit
    lex_chunk, dir_head (chunks.hip)                          test_lex_and_lex_dir_batches_cross_the_grid_limit
    lexr_piece (chunks.hip)                                   test_lex_resume_batch_crosses_the_grid_limit
    write_idat (chunks.hip), twice the limit too              test_write_idat_batch_crosses_the_grid_limit_twice
    wfile_body (chunks.hip)                                   test_write_file_batch_crosses_the_grid_limit, test_compress_batch_crosses_the_grid_limit
    wfile_finish (chunks.hip)                                 test_write_file_batch_crosses_the_grid_limit: jobs 0 and 65535 hold a chunk of two pieces,
                                                              and the host then launches the fold over all N jobs
    unpack, pack (unpack.hip)                                 test_unpack_and_pack_batches_cross_the_grid_limit
    census_kernel, pack_indexed (indexing.hip)                test_census_and_pack_indexed_batches_cross_the_grid_limit
    census_gather / sort_tile / sort_step / write             test_census_wide_batch_crosses_the_grid_limit: jobs 0 and 65535 hold more than 4096 keys,
      (colour_tables.hip)                                     and the host sizes the sort's launches over all N jobs by the most keys of the call
    map_build, map_kernel (colour_tables.hip)                 test_map_batch_crosses_the_grid_limit
    filter (encode.hip)                                       test_filter_batch_crosses_the_grid_limit, test_compress_batch_crosses_the_grid_limit
    scatter (unfilter.hip)                                    test_interlaced_unfilter_crosses_the_grid_limit: spng_unfilter_batch, spng_decode_batch
    overdraw (unfilter.hip)                                   test_overdraw_crosses_the_grid_limit (spng_unfilter_resume_batch: the one entry
                                                              that acts on SPNG_IMAGE_OVERDRAW; an overdraw job per image, so N images)
    gzip_inflate_crc, gzip_deflate_crc (gzip.hip)             test_gzip_trailers_cross_the_grid_limit
    dfl4_block, dfl4_place (deflate.hip)                      test_deflate_level_1_crosses_the_grid_limit, test_compress_batch_crosses_the_grid_limit

What the host's memory planning allows (read in csrc/host_encode.hip and csrc/host_decode.hip):
  deflate, levels 0-7 (deflate_fast_rounds): a one-shot stream of up to 2046 positions takes 2 x 512 bytes of match words, 16 896 of terms,
    256 + 256 of block descriptors and bit counts and 4 x 13 312 + 64 (rounded to 53 504) of block bits: 71 936 bytes.  N such streams are
    4.7 GB, and a group holds what fits the slab budget -- SPNG_CFG_DEFLATE_BYTES, by default half of the free device memory, 288 GB on
    this card --, so N streams are ONE group and dfl4_block / dfl4_place see all of them in one split launch.  (The level-0 streams of
    the gzip test are shorter than 3 bytes: they leave as a stored tail, queue no block, and give those two kernels nothing to do.)
  inflate (cut_into_segments, size_token_pool): a stream is estimated at two token pages of 64 KiB beside its bytes, N streams at 8.6 GB
    of pool, within the default budget of half the free memory; where less is free the host cuts the streams into groups, and the
    gzip launches behind them still see all N.

Not covered, and why:
  launch_rows itself has no host-only test beside tests/test_launch_geometry.py: it lives in csrc/common.hpp behind <hip/hip_runtime.h>
    and ends in hipGetLastError(), so the plain host compiler of tests/geometry.py cannot reach it the way it reaches csrc/geometry.hpp
    without a change to how that shim is built.

Jobs k and 65535 + k share whatever has a period that divides 65535 = 3 x 5 x 17 x 257, and a second launch that redoes the first
one's jobs is seen only where they differ: every job's bytes come from a random pool at an offset of its own, and what is planted goes
by periods that do not divide 65535, counted from the last job where a failure has to lie behind the limit.

Expected values: the restatements of tests/test_gpu_alpha.py, tests/tutorial_ref.py, tests/metadata_ref.py, tests/lex_ref.py,
tests/file_ref.py, tests/write_file_cases.py, tests/indexing_ref.py, oracle/pixels.py and oracle/gzip_wrap.py, the oracle's filter, inflater,
deflater and encoder (tests/pnghelp.py) and zlib.

Wall time of each test on an MI355X, host side included, as pytest --durations reports the calls (the whole module: 9 s, 1.6 s of it
the session's start):
    alpha_and_luminance 0.30 s    text 0.44        lex_and_lex_dir 0.90    lex_resume 0.34       write_idat (twice) 0.46    write_file 0.80
    unpack_and_pack 0.01          census_and_pack_indexed 0.04             census_wide 0.02      map 0.01                   filter 0.13
    interlaced_unfilter 0.15      overdraw 0.04    gzip_trailers 0.47      deflate_level_1 0.99  compress 1.40
The larger figures are the yardsticks' loops on the host: 65 537 calls of the oracle's deflater take a second.  The smallest are what
they look like: a megabyte or two up and down, a call whose kernels have five pixels per job, numpy comparisons, and (census_wide,
map) the jobs of colour_jobs() already made by the test in front of them; lex_resume likewise takes the files of lex_files() as made.
Run on their own, in a fresh process: unpack_and_pack 0.11 s, census_wide 0.04, map 0.04.
"""
import ctypes
import functools
import struct
import sys
import zlib

import numpy as np
import pytest

import file_ref
import indexing_ref as ir
import metadata_ref as mr
import pnghelp as ph
import tutorial_ref as tr
import write_file_cases as wc
from lex_ref import FIELDS, lex_ref
from test_gpu_alpha import RGBA, S, restate

sys.path.insert(0, str(ph.ROOT / "oracle"))
import gzip_wrap as gw  # noqa: E402
import pixels as orc_pixels  # noqa: E402

pytestmark = pytest.mark.gpu

N = 65537            # one more than the grid-row limit plus one: the smallest count whose second launch has a job behind its first
GUARD = 0xEE


# ---- tables of descriptors and results as numpy arrays ------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def dtype_of(ctype):
    """the numpy structured type with the layout of a ctypes structure of the package (pointers as uint64)"""
    def one(t):
        if issubclass(t, ctypes.Array):
            return np.dtype((one(t._type_), (t._length_,)))
        if t is ctypes.c_void_p or issubclass(t, ctypes._Pointer):
            return np.dtype(np.uint64)
        return np.dtype(t)
    names = [n for n, _ in ctype._fields_]
    return np.dtype(dict(names=names, formats=[one(t) for _, t in ctype._fields_], offsets=[getattr(ctype, n).offset for n in names],
                         itemsize=ctypes.sizeof(ctype)))


def table(ctype, n, **columns):
    """n descriptors, a column at a time -> (the ctypes array a C entry takes -- it shares the memory --, the numpy array)"""
    a = np.zeros(n, dtype=dtype_of(ctype))
    for name, v in columns.items():
        a[name] = v
    return (ctype * n).from_buffer(a), a


def rows_of(gpu, res):
    """spng_result[n] -> (n, 6) int64: status, reserved, written, consumed, aux0, aux1"""
    r = np.frombuffer(res, dtype=dtype_of(gpu.Result))
    return np.stack([r["status"].astype(np.int64), r["reserved"].astype(np.int64), r["written"].astype(np.int64), r["consumed"].astype(np.int64),
                     r["aux"][:, 0].astype(np.int64), r["aux"][:, 1].astype(np.int64)], axis=1)


def same_rows(got, want):
    got, want = np.asarray(got, dtype=np.int64), np.asarray(want, dtype=np.int64)
    bad = np.flatnonzero((got != want).reshape(len(got), -1).any(axis=1))
    assert not len(bad), (len(bad), int(bad[0]), got[bad[0]].tolist(), want[bad[0]].tolist())


def same_bytes(got, want, at=None):
    """two byte arrays; at: where the jobs' outputs start, to name the first job that differs"""
    got, want = np.asarray(got).reshape(-1).view(np.uint8), np.asarray(want).reshape(-1).view(np.uint8)
    assert got.shape == want.shape
    bad = np.flatnonzero(got != want)
    if len(bad):
        job = int(np.searchsorted(np.asarray(at), bad[0], side="right") - 1) if at is not None else None
        raise AssertionError(f"{len(bad)} bytes differ, the first at {int(bad[0])} (job {job}): {int(got[bad[0]])}, expected {int(want[bad[0]])}")


def starts(sizes):
    """where slices of `sizes` bytes start when they lie back to back -> int64[n + 1]"""
    return np.concatenate([[0], np.cumsum(np.asarray(sizes, dtype=np.int64))])


def raw_inflate(payload, cap):
    """a raw DEFLATE stream by zlib, in the form oracle/gzip_wrap.py takes its inflater"""
    d = zlib.decompressobj(-15)
    out = d.decompress(payload)
    assert d.eof
    return 0, out, len(payload) - len(d.unused_data), (0, 0)


def fails_on_both_sides(mask):
    """the jobs planted to fail: one in each launch at least, the first and the last of them with a good job beside it"""
    at = np.flatnonzero(mask)
    assert len(at) and at[0] < 65535 <= at[-1] and not mask[at[0] + 1] and not mask[at[-1] - 1]


def test_alpha_and_luminance_batches_cross_the_grid_limit(gpu):
    """one spng_alpha_batch call of N arrays of 3 RGBA<UInt8> pixels, straightened in place, and one spng_luminance_batch call of N
    arrays of 5 pixels to V8: slices of one tensor each; every result reads SPNG_DONE with its own byte and trap counts"""
    s = gpu.load()
    rng = np.random.default_rng(65537)
    px = rng.integers(0, 256, (N * 3, 4), dtype=np.uint8)
    px[rng.random(N * 3) < 0.1, 3] = 0
    want, trapped = restate(px, 8, S)
    # (per array: a component traps where 0 < a < c -- (255 c + a / 2) / a > 255 from c = a + 1 on; held to the restatement's total)
    traps = ((px[:, 3:] > 0) & (px[:, :3] > px[:, 3:])).sum(axis=1).reshape(N, 3).sum(axis=1)
    assert traps.sum() == trapped > N
    d = s.to_device(px.reshape(-1))
    descs = (gpu.AlphaDesc * N)()
    at = d.data_ptr()
    for i in range(N):
        descs[i] = gpu.AlphaDesc(at + 12 * i, at + 12 * i, 3, 8, RGBA, S)
    res = (gpu.Result * N)()
    assert s.lib.spng_alpha_batch(s.ctx, descs, N, None, res) == 0
    assert (d.cpu().numpy().reshape(-1, 4) == want).all()
    got = np.array([(r.status, r.written, r.aux[0]) for r in res])
    assert (got[:, 0] == 0).all() and (got[:, 1] == 12).all() and (got[:, 2] == traps).all()

    px = rng.integers(0, 256, (N * 5, 4), dtype=np.uint8)
    d_in, d_out = s.to_device(px.reshape(-1)), s.to_device(np.full(N * 5, 0xEE, dtype=np.uint8))
    descs = (gpu.LuminanceDesc * N)()
    a, b = d_in.data_ptr(), d_out.data_ptr()
    for i in range(N):
        descs[i] = gpu.LuminanceDesc(a + 20 * i, b + 5 * i, 5, 1)               # (op 1: SPNG_LUMINANCE_V8)
    res = (gpu.Result * N)()
    assert s.lib.spng_luminance_batch(s.ctx, descs, N, None, res) == 0
    assert (d_out.cpu().numpy() == tr.luminance(px)).all()
    got = np.array([(r.status, r.written, r.consumed, r.aux[0]) for r in res])
    assert (got == [0, 5, 20, 0]).all()


# ---- spng_text_batch ----------------------------------------------------------------------------------------------------------
def text_jobs():
    """-> (the inputs back to back, their starts, lengths, ops 0 / 1 / 2 = transcode with room / a byte short / check).  The operation goes
    by i % 3 and the length by (i // 2) % 5: whatever has a period that divides 65535 = 3 x 5 x 17 x 257 is the same for job k of the
    first launch and job k of the second, and a second launch that reads the first one's rows would go unseen.  So job 0 is a byte short
    of nothing (SPNG_DONE) and job 65535 a byte short of 17 bytes: with job 0's result it would write; job 65536 has room for 4095."""
    rng = np.random.default_rng(1)
    i = np.arange(N)
    op, lens = np.array([1, 0, 2])[i % 3], np.array([0, 1, 17, 4095, 4097])[(i // 2) % 5]
    assert len(set(zip(op.tolist(), lens.tolist()))) == 15 and (op[65535], lens[65535], op[65536], lens[65536]) == (1, 17, 0, 4095)
    at = starts(lens)
    data = rng.integers(0, 256, int(at[-1]), dtype=np.uint8)
    for j in np.flatnonzero(op == 2):
        text = data[at[j]:at[j + 1]]
        text &= 0x7f                                           # a text to check is well-formed,
        if (j // 3) % 97 == 0 and lens[j]:                     # but for every 97th: bytes no sequence holds, where and how many by the job
            text[j % lens[j]] = 0xff
            text[(7 * j + 3) % lens[j]] = 0xc0 + j % 2
    return data, at, lens, op


def test_text_batch_crosses_the_grid_limit(gpu):
    """one spng_text_batch call of N texts of 0, 1, 17, 4095 and 4097 bytes (two tiles: the scratch of a job's tiles is its own):
    Latin-1 to UTF-8 a byte short, the same with room, and the UTF-8 check with every 97th text ill-formed"""
    s = gpu.load()
    data, at, lens, op = text_jobs()
    high = np.zeros(N, dtype=np.int64)
    full = np.flatnonzero(lens)
    high[full] = np.add.reduceat((data >= 0x80).astype(np.int64), at[full])
    need = np.where(op < 2, lens + high, 0)
    cap = np.where(op == 0, need, np.maximum(need - 1, 0))
    short = (op < 2) & (cap < need)
    fails_on_both_sides(short)
    out_at = starts(cap + 3)
    want_out = np.full(int(out_at[-1]), GUARD, dtype=np.uint8)
    want = np.zeros((N, 6), dtype=np.int64)
    want[:, 2], want[:, 3] = need, lens
    want[short, 0] = mr.E_OUTPUT_CAPACITY
    for j in range(N):
        text = data[at[j]:at[j + 1]].tobytes()
        if op[j] == 2:
            want[j, 0], want[j, 4], want[j, 5] = mr.check_utf8(text)
        elif not short[j]:
            utf8 = mr.latin1_to_utf8(text)
            assert len(utf8) == need[j]
            want_out[out_at[j]:out_at[j] + need[j]] = np.frombuffer(utf8, dtype=np.uint8)
    assert (want[:, 0] == mr.E_TEXT_ENCODING).sum() > 100      # (the two jobs behind the limit are transcodes: see text_jobs)
    d_in, d_out = s.to_device(data), s.to_device(np.full(int(out_at[-1]), GUARD, dtype=np.uint8))
    descs, _ = table(gpu.TextDesc, N, d_in=d_in.data_ptr() + at[:-1], len=lens, d_out=np.where(op < 2, d_out.data_ptr() + out_at[:-1], 0),
                     out_cap=cap, op=np.where(op < 2, gpu.TEXT_LATIN1_TO_UTF8, gpu.TEXT_CHECK_UTF8))
    res = (gpu.Result * N)()
    assert s.lib.spng_text_batch(s.ctx, descs, N, None, res) == 0
    same_rows(rows_of(gpu, res), want)
    same_bytes(d_out.cpu().numpy(), want_out, out_at)


# ---- the lexer ----------------------------------------------------------------------------------------------------------------
ENTRY = struct.Struct("<IIQiIIIIIB7x")


@functools.lru_cache(maxsize=None)
def lex_files():
    """N files -- signature, an IHDR and a tEXt that name the job, an IDAT of 1 to 40 bytes, IEND; every 101st with a wrong checksum in
    its IDAT -- and what the yardstick lexes from each: -> (files, where the IDAT payload starts, [(Lexed, IDAT bytes)]).  The keyword of
    the tEXt is 3 + i % 7 characters long: the head of job 65535 + k is not the head of job k (7 does not divide 65535)"""
    pool = np.random.default_rng(2).integers(0, 256, N + 64, dtype=np.uint8).tobytes()
    files, idat_at = [], []
    for i in range(N):
        idat = file_ref.chunk(b"IDAT", pool[i:i + 1 + (7 * i) % 40])
        if (N - 2 - i) % 101 == 0:                             # (counted from the end: job 65535 is one)
            idat = idat[:-1] + bytes([idat[-1] ^ 0x40])
        front = file_ref.SIG + file_ref.chunk(b"IHDR", struct.pack(">IIBBBBB", i + 1, 1 + i % 3, 8, 0, 0, 0, 0)) + \
            file_ref.chunk(b"tEXt", b"Job" + b"x" * (i % 7) + b"\0%d" % i + bytes([0xa1 + i % 90]) * (i % 5))
        files.append(front + idat + file_ref.chunk(b"IEND"))
        idat_at.append(len(front) + 8)
    return files, np.array(idat_at), [lex_ref(f, len(f)) for f in files]


def lexed_rows(gpu, infos):
    """spng_lexed[n] -> (n, 18) int64 in the order of lex_ref's fields"""
    a = np.frombuffer(infos, dtype=dtype_of(gpu.Lexed))
    columns = dict({f: a[f] for f in FIELDS if f in a.dtype.names}, aux0=a["aux"][:, 0], aux1=a["aux"][:, 1])
    return np.stack([columns[f].astype(np.int64) for f in FIELDS], axis=1)


def lex_layout(s, gpu, files, lens, copies):
    """the files back to back in one tensor, and `copies` IDAT tensors of a slot per file: as many bytes as its IDAT payload, 8 of guard"""
    at = starts([len(f) for f in files])
    d_png = s.to_device(b"".join(files))
    idat_at = starts(lens + 8)
    d_idat = [s.to_device(np.full(int(idat_at[-1]), GUARD, dtype=np.uint8)) for _ in range(copies)]
    return at, d_png, idat_at, d_idat


def check_idat(got, idat_at, lens, lexed):
    """IDAT slots: the yardstick's bytes in front of idat_len, the guard behind the capacity -- and behind idat_len where the file lexed
    to its end (of a chunk that fails its checksum the payload may have been copied ahead of the sum)"""
    want = np.full(len(got), GUARD, dtype=np.uint8)
    free = np.zeros(len(got), dtype=bool)
    for j, (info, idat) in enumerate(lexed):
        want[idat_at[j]:idat_at[j] + len(idat)] = np.frombuffer(idat, dtype=np.uint8)
        if info.status != 0:
            free[idat_at[j] + len(idat):idat_at[j] + lens[j]] = True
    got = np.where(free, GUARD, got).astype(np.uint8)
    same_bytes(got, want, idat_at)


def test_lex_and_lex_dir_batches_cross_the_grid_limit(gpu):
    """spng_lex_batch and spng_lex_dir_batch over the same N files (every 103rd directory one entry short): the infos of both byte for
    byte the same and field for field the yardstick's, the IDAT bytes, the entries in front of min(chunks, cap), the guard behind them"""
    s = gpu.load()
    files, payload_at, lexed = lex_files()
    lens = np.array([struct.unpack(">I", f[p - 8:p - 4])[0] for f, p in zip(files, payload_at)])
    at, d_png, idat_at, d_idat = lex_layout(s, gpu, files, lens, 2)
    size = ctypes.sizeof(gpu.ChunkEntry)
    assert size == ENTRY.size
    caps = np.where((N - 1 - np.arange(N)) % 103 == 0, 3, 4)     # (job 65536 is one)
    d_ent = s.to_device(np.full(N * 5 * size, GUARD, dtype=np.uint8))
    assert d_ent.data_ptr() % 8 == 0
    infos = []
    for k in range(2):
        descs, _ = table(gpu.FileDesc, N, d_png=d_png.data_ptr() + at[:-1], len=np.diff(at), d_idat=d_idat[k].data_ptr() + idat_at[:-1], idat_cap=lens)
        infos.append((gpu.Lexed * N)())
        if k == 0:
            assert s.lib.spng_lex_batch(s.ctx, descs, N, None, infos[0]) == 0
        else:
            dirs, _ = table(gpu.ChunkDir, N, d_entries=d_ent.data_ptr() + 5 * size * np.arange(N), cap=caps)
            assert s.lib.spng_lex_dir_batch(s.ctx, descs, dirs, N, None, infos[1]) == 0
    assert bytes(infos[0]) == bytes(infos[1])
    same_rows(lexed_rows(gpu, infos[0]), [tuple(info) for info, _ in lexed])
    status = np.array([info.status for info, _ in lexed])
    fails_on_both_sides(status == gpu.E_CHUNK_CHECKSUM)
    assert set(status.tolist()) == {0, gpu.E_CHUNK_CHECKSUM}
    for k in range(2):
        check_idat(d_idat[k].cpu().numpy(), idat_at, lens, lexed)
    want = np.full(N * 5 * size, GUARD, dtype=np.uint8)
    clipped = np.zeros(N, dtype=bool)
    for j, (f, (info, _)) in enumerate(zip(files, lexed)):
        filled = min(info.chunks, int(caps[j]))
        clipped[j] = filled < info.chunks
        raw = b"".join(ENTRY.pack(e.type, e.length, e.offset, e.head.status, e.head.aux, e.head.k, e.head.l, e.head.m, e.head.body_off, e.head.compressed)
                       for e in mr.directory(f, info.chunks)[:filled])
        want[5 * size * j:5 * size * j + len(raw)] = np.frombuffer(raw, dtype=np.uint8)
    fails_on_both_sides(clipped)
    same_bytes(d_ent.cpu().numpy(), want, 5 * size * np.arange(N))


def test_lex_resume_batch_crosses_the_grid_limit(gpu):
    """spng_lex_resume_batch, N states, the same files in two pushes cut inside the IDAT payload: after the first every info is the
    yardstick's for the prefix, after the second for the file, with the IDAT bytes"""
    s = gpu.load()
    files, payload_at, lexed = lex_files()
    lens = np.array([struct.unpack(">I", f[p - 8:p - 4])[0] for f, p in zip(files, payload_at)])
    cut = payload_at + (np.arange(N) * 11) % lens                # (0 ... len - 1 bytes of the payload have arrived)
    at, d_png, idat_at, (d_idat,) = lex_layout(s, gpu, files, lens, 1)
    state = (int(s.lib.spng_lex_state_bytes()) + 15) // 16 * 16
    d_state = s.torch.zeros(N * state, dtype=s.torch.uint8, device=s.tdev)
    state_at = (d_state.data_ptr() + state * np.arange(N)).astype(np.uint64)
    states = (ctypes.c_void_p * N).from_buffer(state_at)
    for push, have in enumerate((cut, np.diff(at))):
        descs, _ = table(gpu.FileDesc, N, d_png=d_png.data_ptr() + at[:-1], len=have, d_idat=d_idat.data_ptr() + idat_at[:-1], idat_cap=lens)
        infos = (gpu.Lexed * N)()
        assert s.lib.spng_lex_resume_batch(s.ctx, descs, states, N, None, infos) == 0
        if push == 0:
            want = [tuple(lex_ref(f[:c], len(f))[0]) for f, c in zip(files, cut)]
            assert {w[0] for w in want} == {gpu.E_TRUNCATED_CHUNK_BODY}
        else:
            want = [tuple(info) for info, _ in lexed]
        same_rows(lexed_rows(gpu, infos), want)
    check_idat(d_idat.cpu().numpy(), idat_at, lens, lexed)


# ---- the writers ----------------------------------------------------------------------------------------------------------------
def test_write_idat_batch_crosses_the_grid_limit_twice(gpu):
    """spng_write_idat_batch over streams of 1 to 40 bytes in chunks of 1, 16 and 17, one in 89 with a byte too little room: a call of N,
    and one of 2 x 65535 + 1, whose third launch has exactly one job"""
    s = gpu.load()
    most = 2 * 65535 + 1
    pool = np.frombuffer(wc.noise(), dtype=np.uint8)
    i = np.arange(most)
    lens, chunk_bytes = 1 + (7 * i) % 40, np.array([1, 16, 17])[i % 3]
    pieces = -(-lens // chunk_bytes)
    need = lens + 12 * pieces
    short = ((N - 1 - i) % 89 == 0) | (i == most - 1)            # (jobs 65536 and 131070 are two)
    cap = need - short
    out_at = starts(cap + 2)
    d_in = s.to_device(pool[:most + 64].copy())
    want_out = np.full(int(out_at[-1]), GUARD, dtype=np.uint8)
    for j in np.flatnonzero(~short):
        want_out[out_at[j]:out_at[j] + need[j]] = np.frombuffer(file_ref.body(wc.noise()[j:j + lens[j]], int(chunk_bytes[j])), dtype=np.uint8)
    want = np.stack([np.where(short, gpu.E_OUTPUT_CAPACITY, 0), 0 * i, need, lens, pieces, 0 * i], axis=1)
    for count in (N, most):
        fails_on_both_sides(short[:count])
        d_out = s.to_device(np.full(int(out_at[-1]), GUARD, dtype=np.uint8))
        descs, _ = table(gpu.ChunkingDesc, count, d_stream=d_in.data_ptr() + i[:count], len=lens[:count], d_out=d_out.data_ptr() + out_at[:count],
                         out_cap=cap[:count], chunk_bytes=chunk_bytes[:count])
        res = (gpu.Result * count)()
        assert s.lib.spng_write_idat_batch(s.ctx, descs, count, None, res) == 0
        same_rows(rows_of(gpu, res), want[:count])
        expect = want_out.copy()
        expect[out_at[count]:] = GUARD
        same_bytes(d_out.cpu().numpy(), expect, out_at)


def test_write_file_batch_crosses_the_grid_limit(gpu):
    """spng_write_file_batch over N files whose IHDR names the job, streams of 1 to 40 bytes in chunks of 1, 16 and 17: one in 89 with
    a byte too little room, one in 83 with its length in a spng_result on the device -- an error there, a length in the job behind it.
    Jobs 0 and 65535 are files of ONE chunk of 1 MiB + 1 and + 7: two pieces, whose sums wfile_finish_kernel folds -- a launch the host makes
    over all N jobs as soon as one file of the call has such a chunk (finish_chunks in write_files, csrc/host_files.hip)"""
    s = gpu.load()
    kw = wc.head_kw()
    cases = []
    for i in range(N):
        src = None
        n = 1 + (7 * i) % 40
        if i in (0, 65535):
            # (of two lengths: the fold of job 65535 with job 0's result row would sum and place the checksum for the wrong length)
            cases.append(wc.make(str(i), 0x7fffffff, wc.PIECE + (7 if i else 1), kw=dict(kw, width=i + 1, height=1 + i % 5), at=i))
            continue
        if (N - 2 - i) % 83 == 0:                              # (counted from the end; the one at 65535 has made way for the long chunk)
            src = (wc.E_STRING_REFERENCE, 12, i, 7)
        elif (N - 2 - i) % 83 == 1:
            src = (wc.DONE, n, 0, 0)
        cases.append(wc.make(str(i), (1, 16, 17)[i % 3], n, kw=dict(kw, width=i + 1, height=1 + i % 5), stream_cap=40 if src else None,
                             short=int((N - 1 - i) % 89 == 0), src=src, at=i))
    out_at = starts([c.out_cap + 5 for c in cases])
    want_out = np.full(int(out_at[-1]), GUARD, dtype=np.uint8)
    want = np.zeros((N, 6), dtype=np.int64)
    for j, c in enumerate(cases):
        row, data = wc.expected(c)
        want[j, 0], want[j, 2:] = row[0], row[1:]
        if data is not None:
            want_out[out_at[j]:out_at[j] + len(data)] = np.frombuffer(data, dtype=np.uint8)
    fails_on_both_sides(want[:, 0] == wc.E_OUTPUT_CAPACITY)
    assert (want[:, 0] == wc.E_STRING_REFERENCE).sum() > 700    # (all in the first launch: the two jobs behind the limit are taken)
    assert want[0, 4] == want[65535, 4] == 1 and (want[0, 3], want[65535, 3]) == (wc.PIECE + 1, wc.PIECE + 7)
    d_in = s.to_device(np.frombuffer(wc.noise(), dtype=np.uint8).copy())
    d_out = s.to_device(np.full(int(out_at[-1]), GUARD, dtype=np.uint8))
    _, upstream = table(gpu.Result, N, status=[c.src[0] if c.src else 0 for c in cases], written=[c.src[1] if c.src else 0 for c in cases])
    upstream["aux"][:, 0], upstream["aux"][:, 1] = [c.src[2] if c.src else 0 for c in cases], [c.src[3] if c.src else 0 for c in cases]
    d_up = s.to_device(upstream.view(np.uint8))
    has_src = np.array([c.src is not None for c in cases])
    i = np.arange(N)
    descs, _ = table(gpu.PngDesc, N, d_stream=d_in.data_ptr() + i, stream_len=np.where(has_src, 0, [c.n for c in cases]),
                     d_stream_result=np.where(has_src, d_up.data_ptr() + ctypes.sizeof(gpu.Result) * i, 0), stream_cap=[c.stream_cap for c in cases],
                     d_out=d_out.data_ptr() + out_at[:-1], out_cap=[c.out_cap for c in cases], chunk_bytes=[c.chunk_bytes for c in cases],
                     width=i + 1, height=1 + i % 5, depth=kw["depth"], channels=kw["channels"])
    res = (gpu.Result * N)()
    assert s.lib.spng_write_file_batch(s.ctx, descs, N, None, res) == 0
    same_rows(rows_of(gpu, res), want)
    same_bytes(d_out.cpu().numpy(), want_out, out_at)


# ---- pixels: unpack and pack ----------------------------------------------------------------------------------------------------
def test_unpack_and_pack_batches_cross_the_grid_limit(gpu):
    """spng_unpack_batch over N rgb8 images of 3 pixels (9 bytes of storage: neighbours are not aligned) to RGBA<UInt16>, and
    spng_pack_batch over N arrays of 3 RGBA<UInt16> pixels back to rgb8, against the oracle over one (N x 3)-pixel array each"""
    s = gpu.load()
    rng = np.random.default_rng(5)
    storage = rng.integers(0, 256, N * 9, dtype=np.uint8)
    d_storage = s.to_device(storage)
    d_out = s.to_device(np.full(N * 26 + 64, GUARD, dtype=np.uint8))      # 24 bytes of pixels, 2 of guard
    assert d_out.data_ptr() % 2 == 0
    i = np.arange(N)
    descs, _ = table(gpu.UnpackDesc, N, d_storage=d_storage.data_ptr() + 9 * i, d_out=d_out.data_ptr() + 26 * i, width=3, height=1, depth=8, channels=3,
                     target=16, layout=gpu.TARGET_RGBA)
    assert s.lib.spng_unpack_batch(s.ctx, descs, N) == 0
    s.sync()                                                   # (no results to wait for: the entry only enqueues)
    want = np.full(N * 26 + 64, GUARD, dtype=np.uint8)
    pixels = orc_pixels.unpack(storage.tobytes(), 8, 3, target=16)
    assert pixels.shape == (N * 3, 4) and pixels.dtype == np.uint16
    want[:N * 26].reshape(N, 26)[:, :24] = pixels.astype("<u2").view(np.uint8).reshape(N, 24)
    same_bytes(d_out.cpu().numpy(), want, 26 * i)

    pixels = rng.integers(0, 65536, (N * 3, 4), dtype=np.uint16)
    d_pixels = s.to_device(pixels.astype("<u2").view(np.uint8).reshape(-1))
    d_back = s.to_device(np.full(N * 11 + 64, GUARD, dtype=np.uint8))     # 9 bytes of storage, 2 of guard
    assert d_pixels.data_ptr() % 2 == 0
    descs, _ = table(gpu.PackDesc, N, d_pixels=d_pixels.data_ptr() + 24 * i, d_storage=d_back.data_ptr() + 11 * i, width=3, height=1, depth=8, channels=3,
                     source=16, layout=gpu.TARGET_RGBA)
    assert s.lib.spng_pack_batch(s.ctx, descs, N) == 0
    s.sync()
    want = np.full(N * 11 + 64, GUARD, dtype=np.uint8)
    want[:N * 11].reshape(N, 11)[:, :9] = np.frombuffer(orc_pixels.pack(pixels, 8, 3), dtype=np.uint8).reshape(N, 9)
    same_bytes(d_back.cpu().numpy(), want, 11 * i)


# ---- pixels: colour tables --------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def colour_jobs():
    """N arrays of 5 RGBA<UInt8> pixels, each drawn from four colours of its own (the first two pixels are the first two colours: two
    keys at least) -> (pixels (N, 5, 4); keys (N, 5); per job: distinct keys, the keys ascending (N, 4), their counts (N, 4); the place
    of every pixel's key in its job's list (N, 5)) -- one np.unique over (job, key), held to indexing_ref on a sample of the jobs"""
    rng = np.random.default_rng(6)
    colours = rng.integers(0, 256, (N, 4, 4), dtype=np.uint8)
    pick = rng.integers(0, 4, (N, 5))
    pick[:, 0], pick[:, 1] = 0, 1
    px = colours[np.arange(N)[:, None], pick]
    keys = ir.keys(px.reshape(-1, 4), 8, ir.RGBA).reshape(N, 5)
    tagged = (np.arange(N, dtype=np.uint64)[:, None] << np.uint64(32)) | keys.astype(np.uint64)
    uniq, inverse, counts = np.unique(tagged.reshape(-1), return_inverse=True, return_counts=True)
    job = (uniq >> np.uint64(32)).astype(np.int64)
    n_keys = np.bincount(job, minlength=N)
    first = starts(n_keys)[:-1]
    place = np.arange(len(uniq)) - first[job]
    table_keys, table_counts = np.zeros((N, 4), dtype=np.uint32), np.zeros((N, 4), dtype=np.uint64)
    table_keys[job, place], table_counts[job, place] = (uniq & np.uint64(0xffffffff)).astype(np.uint32), counts
    where = inverse.reshape(N, 5) - first[:, None]
    assert n_keys.min() >= 2 and n_keys.max() == 4
    for j in SAMPLE:
        k, c = ir.census(px[j], 8, ir.RGBA)
        assert (k == table_keys[j, :n_keys[j]]).all() and (c == table_counts[j, :n_keys[j]]).all()
    return px, keys, n_keys, table_keys, table_counts, where


SAMPLE = list(range(40)) + list(range(65500, N))             # the jobs the vectorised expectations are held to the yardsticks on


def census_crosses(gpu, entry, large=()):
    """a census entry over colour_jobs(): every array has room for four keys, but every 91st for one fewer than it holds.  large: jobs
    that count an array of 5000 random colours instead -- more keys than a tile of the wide census's sort holds"""
    s = gpu.load()
    px, _, n_keys, table_keys, table_counts, _ = colour_jobs()
    i = np.arange(N)
    big_px = np.random.default_rng(13).integers(0, 256, (len(large), 5000, 4), dtype=np.uint8)
    big = [ir.census(p, 8, ir.RGBA) for p in big_px]
    assert all(gpu.CENSUS_WIDE_TILE < len(k) <= 5000 for k, _ in big)
    d_big_px = s.to_device(big_px.reshape(-1))
    d_big_keys, d_big_counts = s.to_device(np.full(len(large) * 5001 * 4 + 64, GUARD, dtype=np.uint8)), s.to_device(np.full(len(large) * 5001 * 8 + 64, GUARD, dtype=np.uint8))
    short = (N - 1 - i) % 91 == 0
    fails_on_both_sides(short)
    cap = np.where(short, n_keys - 1, 4)
    d_px = s.to_device(px.reshape(-1))
    d_keys, d_counts = s.to_device(np.full(N * 20 + 64, GUARD, dtype=np.uint8)), s.to_device(np.full(N * 40 + 64, GUARD, dtype=np.uint8))
    assert d_keys.data_ptr() % 4 == 0 and d_counts.data_ptr() % 8 == 0
    descs, columns = table(gpu.CensusDesc, N, d_pixels=d_px.data_ptr() + 20 * i, count=5, d_keys=d_keys.data_ptr() + 20 * i,
                           d_counts=d_counts.data_ptr() + 40 * i, cap=cap, bits=8, layout=gpu.TARGET_RGBA)
    want = np.zeros((N, 6), dtype=np.int64)
    want[:, 0], want[:, 2], want[:, 3] = np.where(short, gpu.E_OUTPUT_CAPACITY, 0), np.where(short, 0, n_keys), np.where(short, 0, 5)
    for k, j in enumerate(large):
        assert not short[j] and d_big_keys.data_ptr() % 4 == 0 and d_big_counts.data_ptr() % 8 == 0
        columns["d_pixels"][j], columns["count"][j], columns["cap"][j] = d_big_px.data_ptr() + 20000 * k, 5000, 5000
        columns["d_keys"][j], columns["d_counts"][j] = d_big_keys.data_ptr() + 20004 * k, d_big_counts.data_ptr() + 40008 * k
        want[j, 2], want[j, 3] = len(big[k][0]), 5000
    res = (gpu.Result * N)()
    assert entry(s)(s.ctx, descs, N, None, res) == 0
    same_rows(rows_of(gpu, res), want)
    for d_got, width, which in ((d_big_keys, 4, 0), (d_big_counts, 8, 1)):
        want_bytes = np.full(len(large) * 5001 * width + 64, GUARD, dtype=np.uint8)
        for k in range(len(large)):
            raw = big[k][which].astype("<u%d" % width).view(np.uint8)
            want_bytes[5001 * width * k:5001 * width * k + len(raw)] = raw
        same_bytes(d_got.cpu().numpy(), want_bytes, 5001 * width * np.arange(len(large)))
    if len(large):                                             # (their slots among the small arrays' stay guard)
        n_keys = n_keys.copy()
        n_keys[list(large)] = 0
    # behind `written` both arrays are untouched; what an array that overflowed holds in front of its cap is unspecified
    filled = np.arange(4)[None, :] < np.where(short, 0, n_keys)[:, None]
    loose = np.arange(4)[None, :] < np.where(short, cap, 0)[:, None]
    for d_got, width, values in ((d_keys, 4, table_keys), (d_counts, 8, table_counts)):
        got = d_got.cpu().numpy()
        want_bytes = np.full(len(got), GUARD, dtype=np.uint8)
        slots = want_bytes[:N * 5 * width].reshape(N, 5, width)
        slots[:, :4][filled] = values.astype("<u%d" % width).view(np.uint8).reshape(N, 4, width)[filled]
        got = got.copy()
        got[:N * 5 * width].reshape(N, 5, width)[:, :4][loose] = GUARD
        same_bytes(got, want_bytes, 5 * width * i)


def test_census_and_pack_indexed_batches_cross_the_grid_limit(gpu):
    """spng_census_batch over N arrays of 5 pixels of up to four colours each, and spng_pack_indexed_batch over the same arrays, every
    job with its own key table and index bytes, every 7th table without its last key: the pixels of that key miss"""
    census_crosses(gpu, lambda s: s.lib.spng_census_batch)
    s = gpu.load()
    px, keys, n_keys, table_keys, _, where = colour_jobs()
    rng = np.random.default_rng(7)
    i = np.arange(N)
    indices = rng.integers(0, 256, (N, 4), dtype=np.uint8)
    miss = (i % 251).astype(np.uint8)
    map_count = n_keys - ((N - 1 - i) % 7 == 0)
    hit = where < map_count[:, None]
    want_px = np.where(hit, indices[i[:, None], where], miss[:, None]).astype(np.uint8)
    for j in SAMPLE:
        stored, missed = ir.pack_indexed(px[j], 8, ir.RGBA, table_keys[j, :map_count[j]], indices[j, :map_count[j]], miss=int(miss[j]))
        assert (stored == want_px[j]).all() and missed == (~hit[j]).sum()
    fails_on_both_sides((~hit).any(axis=1) & ((N - 1 - i) % 7 == 0))
    d_px, d_keys, d_indices = s.to_device(px.reshape(-1)), s.to_device(table_keys.astype("<u4").view(np.uint8).reshape(-1)), s.to_device(indices.reshape(-1))
    d_out = s.to_device(np.full(N * 7 + 64, GUARD, dtype=np.uint8))       # 5 bytes of storage, 2 of guard
    assert d_keys.data_ptr() % 4 == 0
    descs, _ = table(gpu.PackIndexedDesc, N, d_pixels=d_px.data_ptr() + 20 * i, d_storage=d_out.data_ptr() + 7 * i, d_keys=d_keys.data_ptr() + 16 * i,
                     d_indices=d_indices.data_ptr() + 4 * i, width=5, height=1, map_count=map_count, source=8, layout=gpu.TARGET_RGBA, miss=miss)
    res = (gpu.Result * N)()
    assert s.lib.spng_pack_indexed_batch(s.ctx, descs, N, None, res) == 0
    same_rows(rows_of(gpu, res), np.stack([0 * i, 0 * i, 5 + 0 * i, 5 + 0 * i, (~hit).sum(axis=1), 0 * i], axis=1))
    want = np.full(N * 7 + 64, GUARD, dtype=np.uint8)
    want[:N * 7].reshape(N, 7)[:, :5] = want_px
    same_bytes(d_out.cpu().numpy(), want, 7 * i)


def test_census_wide_batch_crosses_the_grid_limit(gpu):
    """spng_census_wide_batch over the same arrays, but jobs 0 and 65535 count 5000 random colours: more keys than a tile of 4096, so the
    sort behind the count is gather, sort_tile, one sort_step (k = 8192, j = 4096) and a sort_tile again -- launches the host makes over
    all N jobs, sized by the most keys of the call -- and every one of them goes through the split.  A step that missed job 65535 would
    leave the halves of its keys unmerged"""
    census_crosses(gpu, lambda s: s.lib.spng_census_wide_batch, large=(0, 65535))


def test_map_batch_crosses_the_grid_limit(gpu):
    """spng_map_batch over the same arrays to 16-bit values, every job with its own keys, values and miss value: once with every map
    in LDS (no build launch), once with the maps of jobs 0, 1 and N - 1 above MAP_LDS_KEYS -- map_build_kernel runs under the split,
    and the tables of jobs 1 and N - 1 lie at an offset in the scratch, which the second launch must not move"""
    s = gpu.load()
    px, keys, n_keys, table_keys, _, where = colour_jobs()
    rng = np.random.default_rng(8)
    i = np.arange(N)
    values = rng.integers(0, 65536, (N, 4), dtype=np.uint16)
    miss = ((i * 40503) & 0xffff).astype(np.uint16)
    map_count = n_keys - ((N - 2 - i) % 7 == 0)                  # (job 65535 is one whose last key is not in its map)
    hit = where < map_count[:, None]
    small = np.where(hit, values[i[:, None], where], miss[:, None]).astype(np.uint16)
    fails_on_both_sides((~hit).any(axis=1))
    # the large maps: the job's own keys among 600 others
    large = [0, 1, N - 1]
    big_keys = [np.unique(np.concatenate([rng.integers(0, 1 << 32, 600, dtype=np.uint64).astype(np.uint32), table_keys[j, :n_keys[j]]])) for j in large]
    big_values = [rng.integers(0, 65536, len(k), dtype=np.uint16) for k in big_keys]
    assert all(len(k) > gpu.MAP_LDS_KEYS for k in big_keys)
    big_at = starts([len(k) for k in big_keys])
    d_big_keys = s.to_device(np.concatenate(big_keys).astype("<u4").view(np.uint8))
    d_big_values = s.to_device(np.concatenate(big_values).astype("<u2").view(np.uint8))
    d_px, d_keys = s.to_device(px.reshape(-1)), s.to_device(table_keys.astype("<u4").view(np.uint8).reshape(-1))
    d_values = s.to_device(values.astype("<u2").view(np.uint8).reshape(-1))
    assert d_keys.data_ptr() % 4 == 0 and d_values.data_ptr() % 2 == 0 and d_big_keys.data_ptr() % 4 == 0 and d_big_values.data_ptr() % 2 == 0
    miss_bytes = np.zeros((N, 8), dtype=np.uint8)
    miss_bytes[:, :2] = miss.astype("<u2").view(np.uint8).reshape(N, 2)
    for with_large in (False, True):
        want_px, counts, missed = small.copy(), map_count.copy(), (~hit).sum(axis=1)
        key_at, value_at = d_keys.data_ptr() + 16 * i, d_values.data_ptr() + 8 * i
        if with_large:
            for k, j in enumerate(large):
                want_px[j] = big_values[k][np.searchsorted(big_keys[k], keys[j])]
                counts[j], missed[j] = len(big_keys[k]), 0
                key_at[j], value_at[j] = d_big_keys.data_ptr() + 4 * big_at[k], d_big_values.data_ptr() + 2 * big_at[k]
        d_out = s.to_device(np.full(N * 12 + 64, GUARD, dtype=np.uint8))  # 10 bytes of values, 2 of guard
        assert d_out.data_ptr() % 2 == 0
        descs, _ = table(gpu.MapDesc, N, d_pixels=d_px.data_ptr() + 20 * i, d_out=d_out.data_ptr() + 12 * i, d_keys=key_at, d_values=value_at, count=5,
                         map_count=counts, source=8, layout=gpu.TARGET_RGBA, value_bytes=2, miss=miss_bytes)
        res = (gpu.Result * N)()
        assert s.lib.spng_map_batch(s.ctx, descs, N, None, res) == 0
        same_rows(rows_of(gpu, res), np.stack([0 * i, 0 * i, 10 + 0 * i, 5 + 0 * i, missed, 0 * i], axis=1))
        want = np.full(N * 12 + 64, GUARD, dtype=np.uint8)
        want[:N * 12].reshape(N, 12)[:, :10] = want_px.astype("<u2").view(np.uint8).reshape(N, 10)
        same_bytes(d_out.cpu().numpy(), want, 12 * i)


# ---- scanlines ------------------------------------------------------------------------------------------------------------------
def test_filter_batch_crosses_the_grid_limit(gpu):
    """spng_filter_batch over N gray8 images of 2 x 2 pixels: 6 bytes of filtered rows each, the oracle's filter per image"""
    s = gpu.load()
    storage = np.random.default_rng(9).integers(0, 256, N * 4, dtype=np.uint8)
    want = np.full(N * 7 + 64, GUARD, dtype=np.uint8)                     # 6 bytes of rows, 1 of guard
    rows = np.zeros(N * 6, dtype=np.uint8)
    orc = ph.oracle()
    assert orc.orc_inflated_size(2, 2, 8, 1, 0) == 6
    for j in range(N):
        orc.orc_filter(storage.ctypes.data + 4 * j, 2, 2, 8, 1, 0, rows.ctypes.data + 6 * j)
    assert rows[:6].tobytes() == ph.orc_filter(storage[:4], 2, 2, 8, 1, False) and len(set(rows[::3].tolist())) > 1
    want[:N * 7].reshape(N, 7)[:, :6] = rows.reshape(N, 6)
    d_storage, d_rows = s.to_device(storage), s.to_device(np.full(N * 7 + 64, GUARD, dtype=np.uint8))
    i = np.arange(N)
    descs, _ = table(gpu.ImageDesc, N, d_rows=d_rows.data_ptr() + 7 * i, rows_cap=6, d_storage=d_storage.data_ptr() + 4 * i, width=2, height=2, depth=8,
                     channels=1)
    res = (gpu.Result * N)()
    assert s.lib.spng_filter_batch(s.ctx, descs, N, None, res) == 0
    same_rows(rows_of(gpu, res), np.stack([0 * i, 0 * i, 6 + 0 * i, 0 * i, 0 * i, 0 * i], axis=1))
    same_bytes(d_rows.cpu().numpy(), want, 7 * i)


# 8 x 8 gray8, Adam7: (bx, by, sx, sy, w, h, where the sub-image starts in the scanline stream) of the seven passes, none of them empty
ADAM7 = ((0, 0, 8, 8, 1, 1, 0), (4, 0, 8, 8, 1, 1, 2), (0, 4, 4, 8, 2, 1, 4), (2, 0, 4, 4, 2, 2, 7), (0, 2, 2, 4, 4, 2, 13), (1, 0, 2, 2, 4, 4, 23),
         (0, 1, 1, 2, 8, 4, 43))
U8 = 79                                                      # bytes of its scanline stream
IMAGES = 9363                                                # x 7 scatter jobs = 65541: the last image's jobs lie on both sides of the limit


def interlaced(n, seed):
    """n images of known pixels -> (pixels (n, 8, 8), their scanline streams (n, 79), every scanline of filter type 0)"""
    px = np.random.default_rng(seed).integers(0, 256, (n, 8, 8), dtype=np.uint8)
    rows = np.zeros((n, U8), dtype=np.uint8)
    for bx, by, sx, sy, w, h, off in ADAM7:
        for y in range(h):
            rows[:, off + y * (w + 1) + 1:off + (y + 1) * (w + 1)] = px[:, by + y * sy, bx::sx]
    return px, rows


def assigned(px, lengths, fill=GUARD):
    """storage after the scanlines that are whole within `lengths` bytes of each stream have been assigned; `fill` elsewhere"""
    out = np.full(px.shape, fill, dtype=np.uint8)
    for bx, by, sx, sy, w, h, off in ADAM7:
        whole = np.clip((lengths - off) // (w + 1), 0, h)
        for y in range(h):
            there = whole > y
            out[there, by + y * sy, bx::sx] = px[there, by + y * sy, bx::sx]
    return out


def image_table(gpu, n, d_rows, d_storage, **more):
    i = np.arange(n)
    return table(gpu.ImageDesc, n, d_rows=d_rows.data_ptr() + U8 * i, rows_cap=U8, d_storage=d_storage.data_ptr() + 67 * i, width=8, height=8, depth=8,
                 channels=1, interlaced=1, **more)


def check_storage(d_storage, want_px, n):
    want = np.full(n * 67 + 64, GUARD, dtype=np.uint8)                    # 64 bytes of storage, 3 of guard
    want[:n * 67].reshape(n, 67)[:, :64] = want_px.reshape(n, 64)
    same_bytes(d_storage.cpu().numpy(), want, 67 * np.arange(n))


def test_interlaced_unfilter_crosses_the_grid_limit(gpu):
    """spng_unfilter_batch over 9363 interlaced images -- 65 541 scatter jobs --, one in 79 with a scanline stream that ends early: its
    later scanlines stay unassigned.  Then the same images as zlib streams through spng_decode_batch, twice, one in 79 with a wrong
    Adler-32: the scatter looks its image's status up through job_image[] and leaves that storage alone"""
    s = gpu.load()
    n = IMAGES
    assert gpu.inflated_size(8, 8, 8, 1, True) == U8 and 7 * (n - 1) < 65535 < 7 * n
    px, rows = interlaced(n, 10)
    i = np.arange(n)
    short = (n - 1 - i) % 79 == 0
    lengths = np.where(short, 23 + (5 * i) % 56, U8)
    d_rows, d_storage = s.to_device(rows.reshape(-1)), s.to_device(np.full(n * 67 + 64, GUARD, dtype=np.uint8))
    d_len = s.torch.tensor(lengths.tolist(), dtype=s.torch.int64, device=s.tdev)
    descs, _ = image_table(gpu, n, d_rows, d_storage)
    res = (gpu.Result * n)()
    assert s.lib.spng_unfilter_batch(s.ctx, descs, n, d_len.data_ptr(), None, res) == 0
    same_rows(rows_of(gpu, res), np.stack([0 * i, 0 * i, lengths, 0 * i, 0 * i, 0 * i], axis=1))
    want_px = assigned(px, lengths)
    assert (want_px[~short] == px[~short]).all() and (want_px[n - 1] != px[n - 1]).any()
    check_storage(d_storage, want_px, n)

    # Every scatter job behind the limit belongs to the last image.  With that image's checksum wrong, its storage stays as it was
    # whatever jobs the second launch runs, but the launch has to look up the right status (job_image[] moved on); with the image in
    # front of it wrong instead, the second launch has to run the right jobs.  So twice, one call each.
    good = [zlib.compress(r.tobytes(), 1 + j % 9) for j, r in enumerate(rows)]
    for last in (n - 1, n - 2):
        wrong = (last - i) % 79 == 0
        streams = [z[:-1] + bytes([z[-1] ^ 0x10]) if w else z for z, w in zip(good, wrong)]
        at = starts([len(z) for z in streams])
        d_idat, d_scratch = s.to_device(b"".join(streams)), s.to_device(np.full(n * U8, GUARD, dtype=np.uint8))
        d_storage = s.to_device(np.full(n * 67 + 64, GUARD, dtype=np.uint8))
        descs, _ = image_table(gpu, n, d_scratch, d_storage, d_idat=d_idat.data_ptr() + at[:-1], idat_len=np.diff(at), format=gpu.FORMAT_ZLIB)
        res = (gpu.Result * n)()
        assert s.lib.spng_decode_batch(s.ctx, descs, n, None, res) == 0
        want = np.zeros((n, 6), dtype=np.int64)
        for j, z in enumerate(streams):
            st, out, consumed, aux = ph.orc_inflate(z, 0, U8)
            want[j] = st, 0, len(out), consumed, aux[0], aux[1]
        assert ((want[:, 0] == gpu.E_STREAM_CHECKSUM) == wrong).all() and (want[~wrong, 0] == 0).all() and wrong[last] and not wrong[0]
        got = rows_of(gpu, res)
        got[:, 1] = 0                                          # (reserved: which of the two inflaters took the stream)
        got[wrong, 3] = want[wrong, 3]                         # (consumed: of a stream that fails, as tests/test_gpu_decode.py has it)
        same_rows(got, want)
        check_storage(d_storage, np.where(wrong[:, None, None], GUARD, px).astype(np.uint8), n)
    s.trim()


def test_overdraw_crosses_the_grid_limit(gpu):
    """spng_unfilter_resume_batch with SPNG_IMAGE_OVERDRAW over N interlaced images, each pushed up to a scanline count of its own:
    an overdraw job per image.  Expected: oracle/pixels.py's overdrawn(), once per scanline count, on an image of pixel numbers"""
    s = gpu.load()
    px, rows = interlaced(N, 11)
    i = np.arange(N)
    now = np.array([2, 7, 13, 23, 33, 56])[i % 6]              # bytes pushed: 1, 3, 5, 7, 9 and 12 whole scanlines, the last with 4 bytes of the next
    scanlines = {2: 1, 7: 3, 13: 5, 23: 7, 33: 9, 56: 12}
    want_px = np.empty((N, 64), dtype=np.uint8)
    numbers = np.arange(64, dtype=np.uint8).reshape(8, 8, 1)
    for length, k in scanlines.items():
        source = orc_pixels.overdrawn(numbers, k, fill=255).reshape(64)          # which pixel every pixel shows; 255: none yet
        mine = now == length
        want_px[mine] = np.where(source == 255, GUARD, px.reshape(N, 64)[mine][:, np.minimum(source, 63)])
    d_rows, d_work = s.to_device(rows.reshape(-1)), s.to_device(np.full(N * U8, GUARD, dtype=np.uint8))
    d_storage = s.to_device(np.full(N * 67 + 64, GUARD, dtype=np.uint8))
    descs, _ = image_table(gpu, N, d_rows, d_storage, reserved=gpu.IMAGE_OVERDRAW)
    work_at = (d_work.data_ptr() + U8 * i).astype(np.uint64)
    prev, now_len = np.zeros(N, dtype=np.uint64), now.astype(np.uint64)
    u64p = ctypes.POINTER(ctypes.c_uint64)
    res = (gpu.Result * N)()
    assert s.lib.spng_unfilter_resume_batch(s.ctx, descs, (ctypes.c_void_p * N).from_buffer(work_at), prev.ctypes.data_as(u64p), now_len.ctypes.data_as(u64p),
                                            N, None, res) == 0
    whole = np.where(now == 56, 52, now)
    same_rows(rows_of(gpu, res), np.stack([0 * i, 0 * i, whole, whole, 0 * i, 0 * i], axis=1))
    check_storage(d_storage, want_px, N)


# ---- streams ----------------------------------------------------------------------------------------------------------------------
def test_gzip_trailers_cross_the_grid_limit(gpu):
    """spng_inflate_batch over N gzip members of 1 to 20 bytes, stored and fixed-code blocks in turn, every 107th with a wrong CRC-32 (and
    a zlib stream in every 4099th place);
    spng_deflate_batch(gzip) at level 0 over N inputs of 0 to 2 bytes: every member inflates (zlib, wbits 31: header, CRC-32 and size
    checked) to its input"""
    s = gpu.load()
    pool = np.frombuffer(wc.noise(), dtype=np.uint8)[:N + 64].tobytes()
    i = np.arange(N)
    bad = (N - 1 - i) % 107 == 0
    fails_on_both_sides(bad)
    plain = i % 4099 == 0                                      # zlib streams among the members, job 0 one of them: they have no gzip trailer,
    members, want = [], np.zeros((N, 6), dtype=np.int64)       # and a launch that looked at job 0's header for job 65535 would not sum that member
    for j in range(N):
        data = pool[j:j + 1 + (3 * j) % 20]
        if plain[j]:
            members.append(zlib.compress(data))
            want[j] = 0, 0, len(data), len(members[-1]), 0, 0
            continue
        if j % 2:
            c = zlib.compressobj(9, zlib.DEFLATED, -15)
            raw = c.compress(data) + c.flush()
        else:
            raw = b"\x01" + struct.pack("<HH", len(data), len(data) ^ 0xffff) + data
        crc = zlib.crc32(data) ^ (1 << j % 32 if bad[j] else 0)
        members.append(gw.HEADER + raw + struct.pack("<II", crc, len(data)))
        st, out, consumed, aux = gw.inflate(members[-1], raw_inflate)
        assert out == data and st == (gpu.E_STREAM_CHECKSUM if bad[j] else 0)
        want[j] = st, 0, len(out), consumed, aux[0], aux[1]
    at, lens = starts([len(m) for m in members]), want[:, 2]
    out_at = starts(lens + 3)
    d_in, d_out = s.to_device(b"".join(members)), s.to_device(np.full(int(out_at[-1]) + 64, GUARD, dtype=np.uint8))
    assert plain[0] and not bad[plain].any() and not plain[65535:].any()
    descs, _ = table(gpu.StreamDesc, N, d_src=d_in.data_ptr() + at[:-1], src_len=np.diff(at), d_dst=d_out.data_ptr() + out_at[:-1], dst_cap=lens,
                     format=np.where(plain, gpu.FORMAT_ZLIB, gpu.FORMAT_GZIP))
    res = (gpu.Result * N)()
    assert s.lib.spng_inflate_batch(s.ctx, descs, N, None, res) == 0
    got = rows_of(gpu, res)
    got[:, 1] = 0                                              # (reserved: which of the two inflaters took the stream)
    got[bad, 3] = want[bad, 3]                                 # (consumed: of a stream that fails, as tests/test_gpu_decode.py has it)
    same_rows(got, want)
    want_out = np.full(int(out_at[-1]) + 64, GUARD, dtype=np.uint8)
    for j in range(N):
        want_out[out_at[j]:out_at[j] + lens[j]] = np.frombuffer(pool[j:j + lens[j]], dtype=np.uint8)
    same_bytes(d_out.cpu().numpy(), want_out, out_at)
    s.trim()

    lens = (5 * i) % 3
    d_in, d_out = s.to_device(np.frombuffer(pool, dtype=np.uint8).copy()), s.to_device(np.full(N * 40 + 64, GUARD, dtype=np.uint8))
    descs, _ = table(gpu.StreamDesc, N, d_src=d_in.data_ptr() + i, src_len=lens, d_dst=d_out.data_ptr() + 40 * i, dst_cap=36, format=gpu.FORMAT_GZIP)
    levels = (ctypes.c_int32 * N)()
    res = (gpu.Result * N)()
    assert s.lib.spng_deflate_batch(s.ctx, descs, levels, N, None, res) == 0
    got, out = rows_of(gpu, res), d_out.cpu().numpy()
    assert (got[:, 2] <= 36).all()
    same_rows(got, np.stack([0 * i, 0 * i, got[:, 2], lens, 0 * i, 0 * i], axis=1))
    slots = out[:N * 40].reshape(N, 40)
    assert (slots[np.arange(40)[None, :] >= got[:, 2][:, None]] == GUARD).all() and (out[N * 40:] == GUARD).all()
    for j in range(N):
        d = zlib.decompressobj(31)
        assert d.decompress(slots[j, :got[j, 2]].tobytes()) == pool[j:j + lens[j]] and d.eof and not d.unused_data, j
    s.trim()


def test_deflate_level_1_crosses_the_grid_limit(gpu):
    """spng_deflate_batch at level 1 over N inputs of 6 to 11 bytes, each with a repeat in it: one group of the host, so that
    dfl4_block_kernel and dfl4_place_kernel run under the split with a block per stream; every stream is the oracle's, byte for byte"""
    s = gpu.load()
    pool = np.frombuffer(wc.noise(), dtype=np.uint8)[:N + 64]
    i = np.arange(N)
    lens = 6 + i % 6
    inputs = np.zeros((N, 11), dtype=np.uint8)
    for k in range(11):
        inputs[:, k] = pool[i + k % 4]                         # (bytes 4 ... of an input repeat its first four)
    wants = [ph.orc_deflate(inputs[j, :lens[j]].tobytes(), 1) for j in range(N)]
    sizes = np.array([len(w) for w in wants])
    assert sizes.max() <= 40
    d_in, d_out = s.to_device(inputs.reshape(-1)), s.to_device(np.full(N * 44 + 64, GUARD, dtype=np.uint8))
    descs, _ = table(gpu.StreamDesc, N, d_src=d_in.data_ptr() + 11 * i, src_len=lens, d_dst=d_out.data_ptr() + 44 * i, dst_cap=40, format=gpu.FORMAT_ZLIB)
    levels = (ctypes.c_int32 * N)(*([1] * N))
    res = (gpu.Result * N)()
    assert s.lib.spng_deflate_batch(s.ctx, descs, levels, N, None, res) == 0
    same_rows(rows_of(gpu, res), np.stack([0 * i, 0 * i, sizes, lens, 0 * i, 0 * i], axis=1))
    want = np.full(N * 44 + 64, GUARD, dtype=np.uint8)
    for j, w in enumerate(wants):
        want[44 * j:44 * j + len(w)] = np.frombuffer(w, dtype=np.uint8)
    same_bytes(d_out.cpu().numpy(), want, 44 * i)
    s.trim()


def test_compress_batch_crosses_the_grid_limit(gpu):
    """spng_compress_batch at level 1 over N gray8 images of 2 x 2 pixels into files with IDAT chunks of 1, 16 and 17 bytes, one in 89
    with a byte too little room: the filter, the deflater and the writer each under the split, the writer reading the encoder's results
    on the device.  Expected: the oracle's encoder per image, framed by tests/file_ref.py"""
    s = gpu.load()
    storage = np.random.default_rng(12).integers(0, 256, N * 4, dtype=np.uint8)
    i = np.arange(N)
    chunk_bytes = np.array([1, 16, 17])[i % 3]
    short = (N - 1 - i) % 89 == 0
    fails_on_both_sides(short)
    orc = ph.oracle()
    stream, written = np.zeros(64, dtype=np.uint8), ctypes.c_size_t(0)
    files, want = [], np.zeros((N, 6), dtype=np.int64)
    for j in range(N):
        assert orc.orc_encode(storage.ctypes.data + 4 * j, 2, 2, 8, 1, 0, 0, 1, stream.ctypes.data, 64, ctypes.byref(written)) == 0
        z = stream[:written.value].tobytes()
        files.append(file_ref.write(z, int(chunk_bytes[j]), 2, 2, 8, 1))
        want[j] = (gpu.E_OUTPUT_CAPACITY, 0, len(files[j]), 0, 0, 0) if short[j] else (0, 0, len(files[j]), len(z), -(-len(z) // chunk_bytes[j]), 0)
    assert zlib.decompress(z) == ph.orc_filter(storage[-4:], 2, 2, 8, 1, False) and max(want[:, 3]) <= 36
    cap = np.array([len(f) for f in files]) - short
    out_at = starts(cap + 3)
    want_out = np.full(int(out_at[-1]) + 64, GUARD, dtype=np.uint8)
    for j in np.flatnonzero(~short):
        want_out[out_at[j]:out_at[j] + len(files[j])] = np.frombuffer(files[j], dtype=np.uint8)
    d_storage, d_rows, d_idat = s.to_device(storage), s.empty(N * 6), s.to_device(np.full(N * 40 + 64, GUARD, dtype=np.uint8))
    d_out = s.to_device(np.full(int(out_at[-1]) + 64, GUARD, dtype=np.uint8))
    images, _ = table(gpu.ImageDesc, N, d_idat=d_idat.data_ptr() + 40 * i, idat_len=36, d_rows=d_rows.data_ptr() + 6 * i, rows_cap=6,
                      d_storage=d_storage.data_ptr() + 4 * i, width=2, height=2, depth=8, channels=1, format=gpu.FORMAT_ZLIB)
    descs, _ = table(gpu.PngDesc, N, d_out=d_out.data_ptr() + out_at[:-1], out_cap=cap, chunk_bytes=chunk_bytes)
    res = (gpu.Result * N)()
    assert s.lib.spng_compress_batch(s.ctx, images, descs, 1, N, None, res) == 0
    same_rows(rows_of(gpu, res), want)
    same_bytes(d_out.cpu().numpy(), want_out, out_at)
    assert (d_idat.cpu().numpy()[:N * 40].reshape(N, 40)[:, 36:] == GUARD).all()
    s.trim()
