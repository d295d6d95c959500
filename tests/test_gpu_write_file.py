"""GPU: spng_write_file_batch over the emulator's case table (tests/write_file_cases.py: the bytes from tests/file_ref.py), every case alone
and all of them as one batch; the asynchronous form (d_results only, then one read); and the round trip -- the written files through
spng_lex_batch to SPNG_DONE with the stream back out.  Output and stream buffers sit at the residues mod 16 the cases name."""
import ctypes

import pytest

import write_file_cases as wc

pytestmark = pytest.mark.gpu


def at_residue(s, n, residue, data=None):
    """a device buffer of n bytes whose address is `residue` mod 16 (a view into a longer tensor)"""
    t = s.empty(n + 32)
    off = (residue - t.data_ptr()) % 16
    v = t[off:off + max(n, 1)]
    if data:
        v[:len(data)] = s.to_device(data)
    return v


def lay_out(s, gpu, cases):
    """-> (PngDesc array, what must stay alive, the output views)"""
    descs, keep, outs = (gpu.PngDesc * len(cases))(), [], []
    for i, c in enumerate(cases):
        kw = dict(c.kw)
        d, k = gpu.png_desc((kw.pop("width"), kw.pop("height")), kw.pop("depth"), kw.pop("channels"), chunk_bytes=c.chunk_bytes, **kw)
        src, out = at_residue(s, len(c.buffer), c.stream_res, c.buffer), at_residue(s, c.out_cap, c.out_res)
        out.fill_(0xEE)
        d.d_stream, d.stream_len, d.stream_cap, d.d_out, d.out_cap = src.data_ptr(), c.n, c.stream_cap, out.data_ptr(), c.out_cap
        if c.src is not None:
            r = gpu.Result(c.src[0], 0, c.src[1], 0, (ctypes.c_uint64 * 2)(c.src[2], c.src[3]))
            dr = s.to_device(bytes(r))
            d.d_stream_result, d.stream_len = dr.data_ptr(), 0
            keep.append(dr)
        descs[i] = d
        keep += [k, src]
        outs.append(out)
    return descs, keep, outs


def check(s, cases, results, outs):
    for c, r, out in zip(cases, results, outs):
        kept = r.written if r.status == wc.DONE else 0
        host = bytes(out.cpu().numpy())
        assert host[kept:c.out_cap] == b"\xee" * (c.out_cap - kept), ("bytes behind the file were written", c.name)
        wc.check_row(c, (r.status, r.written, r.consumed, r.aux[0], r.aux[1]), host[:kept])


@pytest.fixture(scope="module")
def table():
    return wc.length_cases() + wc.residue_cases() + wc.capacity_cases() + wc.source_cases() + wc.fold_cases()


def test_every_case_alone(gpu, table):
    s = gpu.load()
    for c in table:
        descs, keep, outs = lay_out(s, gpu, [c])
        check(s, [c], s.write_file_batch(descs), outs)


def test_all_cases_as_one_batch(gpu, table):
    s = gpu.load()
    cases = table + wc.mixed_batch()
    descs, keep, outs = lay_out(s, gpu, cases)
    check(s, cases, s.write_file_batch(descs), outs)


def test_asynchronous_form_and_the_round_trip_through_the_lexer(gpu):
    """d_results only: the call returns with the kernels enqueued; one read afterwards.  Then every file it wrote is lexed on the
    device: SPNG_DONE, the IDAT bytes are the stream"""
    s = gpu.load()
    cases = wc.mixed_batch()
    descs, keep, outs = lay_out(s, gpu, cases)
    d_results = s.torch.zeros(len(cases) * ctypes.sizeof(gpu.Result), dtype=s.torch.uint8, device=s.tdev)
    assert s.write_file_batch(descs, d_results=d_results, wait=False) is None
    s.sync()
    results = list((gpu.Result * len(cases)).from_buffer_copy(bytes(d_results.cpu().numpy())))
    check(s, cases, results, outs)
    done = [(c, r, out) for c, r, out in zip(cases, results, outs) if r.status == wc.DONE]
    assert len(done) > len(cases) // 2
    infos, idats = s.lex_batch([bytes(out[:r.written].cpu().numpy()) for c, r, out in done])
    for (c, r, out), info, idat in zip(done, infos, idats):
        assert (info.status, info.consumed, info.idat_len, info.width, info.height) == (wc.DONE, r.written, r.consumed, c.kw["width"], c.kw["height"]), c.name
        assert idat == c.buffer[:r.consumed] and info.chunks == r.aux[0] + 2 + len(c.kw["before"]) + len(c.kw["after"]) + \
            sum(x is not None for x in wc.file_ref.derived(c.kw["depth"], c.kw["channels"], c.kw["indexed"], c.kw["bgr"], c.kw["palette"], c.kw["key"], c.kw["fill"])) + c.kw["bgr"], c.name


def test_refusals_reach_the_caller(gpu):
    """what file_head refuses is the call's status, before anything is launched"""
    s = gpu.load()
    c = wc.make("refused", 16, 40)
    for change in (dict(chunk_bytes=0), dict(chunk_bytes=0x80000000), dict(width=0)):
        descs, keep, outs = lay_out(s, gpu, [c])
        for k, v in change.items():
            setattr(descs[0], k, v)
        res = (gpu.Result * 1)()
        assert s.lib.spng_write_file_batch(s.ctx, descs, 1, None, res) == gpu.E_ARGUMENT
        assert s.lib.spng_file_bound(ctypes.byref(descs[0]), 40) == 0
    descs, keep, outs = lay_out(s, gpu, [c])
    assert s.lib.spng_file_bound(ctypes.byref(descs[0]), 40) == c.out_cap
