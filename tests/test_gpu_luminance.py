"""GPU checks of spng_luminance_batch / spng_luminance (COMPUTE_LUMINANCE of the reference's Snippets/PNG/BasicEncoding.swift:63-71) and of
the mirror's PNG.luminance.  Expected values come from tests/tutorial_ref.py, the formula in numpy's binary64 in the tutorial's
association with halves away from zero, which tests/test_tutorial_streams.py holds against the file the tutorial wrote.  Byte for
byte over all 2^24 colours: 38 of them land on an exact half, 97 change in float, 2 with the products associated the other way."""
import ctypes

import numpy as np
import pytest

import tutorial_ref as tr

pytestmark = pytest.mark.gpu

V8, VA8 = 1, 2                                                  # (the op is the bytes of a pixel coming out)
COUNTS = [0, 1, 3, 15, 16, 17, 63, 64, 65, 4097]
OFFSETS = [0, 1, 4, 15]


def convert(op, data: bytes) -> bytes:
    px = np.frombuffer(data, dtype=np.uint8).reshape(-1, 4)
    l = tr.luminance(px)
    return l.tobytes() if op == V8 else np.stack([l, px[:, 3]], axis=1).tobytes()


def layout(jobs, in_off, out_off):
    """jobs: [(op, input bytes)] -> slots of two buffers that start `in_off` / `out_off` bytes behind a 16-byte boundary, 64 bytes
    apart at least: ([(at, bytes)] in, [(at, bytes)] out, the input buffer, the expected output buffer over a poison of 0xEE)"""
    ins, outs, ipos, opos = [], [], 0, 0
    for op, data in jobs:
        n = len(data) // 4
        ins.append((ipos + in_off, len(data)))
        outs.append((opos + out_off, n * op))
        ipos = (ipos + in_off + len(data) + 64 + 15) & ~15
        opos = (opos + out_off + n * op + 64 + 15) & ~15
    host = np.zeros(ipos + 16, dtype=np.uint8)
    want = np.full(opos + 16, 0xEE, dtype=np.uint8)
    for (op, data), (ia, il), (oa, ol) in zip(jobs, ins, outs):
        host[ia:ia + il] = np.frombuffer(data, dtype=np.uint8)
        want[oa:oa + ol] = np.frombuffer(convert(op, data), dtype=np.uint8)
    return ins, outs, host, want


def run_batch(s, jobs, in_off=0, out_off=0):
    """every job one desc of ONE spng_luminance_batch call; checks status, byte counts, aux, the pixels and every byte outside the
    outputs (guard bytes on both sides of each)"""
    ins, outs, host, want = layout(jobs, in_off, out_off)
    d_in, d_out = s.to_device(host), s.to_device(np.full_like(want, 0xEE))
    assert d_in.data_ptr() % 16 == 0 and d_out.data_ptr() % 16 == 0
    _, res = s.luminance_batch([d_in[a:a + n] for a, n in ins], [op for op, _ in jobs], outs=[d_out[a:a + n] for a, n in outs])
    back = d_out.cpu().numpy()
    for r, (_, il), (_, ol) in zip(res, ins, outs):
        assert (r.status, r.written, r.consumed, r.aux[0], r.aux[1]) == (0, ol, il, 0, 0)
    bad = np.flatnonzero(back != want)
    assert bad.size == 0, ([op for op, _ in jobs], in_off, out_off, bad[:8], back[bad[:8]], want[bad[:8]])


@pytest.fixture(scope="module")
def every_colour():
    """all 2^24 colours as (n, 4) uint8 -- alpha the low byte of the index -- and their luminance by the restatement, computed once"""
    c = np.arange(1 << 24, dtype=np.uint32)
    px = np.stack([c & 255, (c >> 8) & 255, (c >> 16) & 255, c & 255], axis=1).astype(np.uint8)
    want = np.concatenate([tr.luminance(px[at:at + (1 << 22)]) for at in range(0, 1 << 24, 1 << 22)])
    px.setflags(write=False)
    want.setflags(write=False)
    return px, want


@pytest.mark.parametrize("op", [V8, VA8])
def test_every_colour_in_one_call(gpu, every_colour, op):
    """64 MiB in, 16 (32) MiB out: the float root of the device (v_sqrt_f32) under every x the formula can produce"""
    s = gpu.load()
    px, want = every_colour
    d_in = s.to_device(px.reshape(-1).copy())                  # (the shared array stays read-only)
    (d_out,), (r,) = s.luminance_batch([d_in], op)
    assert (r.status, r.written, r.consumed, r.aux[0]) == (0, op << 24, 4 << 24, 0)
    got = d_out.cpu().numpy().reshape(-1, op)
    bad = np.flatnonzero(got[:, 0] != want)
    assert bad.size == 0, (bad.size, px[bad[:4]], got[bad[:4], 0], want[bad[:4]])
    if op == VA8:
        assert np.array_equal(got[:, 1], px[:, 3])


@pytest.mark.parametrize("op", [V8, VA8])
def test_shapes_and_offsets(gpu, op):
    """pixel counts around the 16-byte access, the wave and the block, in one call each, for every pair of input and output offsets
    of 0, 1, 4 and 15 bytes from a 16-byte boundary (only (0, 0) takes the 16-byte path)"""
    s = gpu.load()
    rng = np.random.default_rng(op)
    jobs = [(op, rng.integers(0, 256, 4 * n, dtype=np.uint8).tobytes()) for n in COUNTS]
    for in_off in OFFSETS:
        for out_off in OFFSETS:
            run_batch(s, jobs, in_off, out_off)


def mixed_jobs():
    rng = np.random.default_rng(8)
    return [(op, rng.integers(0, 256, 4 * n, dtype=np.uint8).tobytes())
            for op, n in ((VA8, 4099), (V8, 0), (V8, 70001), (VA8, 1030), (V8, 16), (VA8, 7), (V8, 65537), (VA8, 64))]


def test_a_mixed_batch(gpu):
    """eight descs in one call, both operations, several lengths, an empty one, aligned and not: each result equals its array alone"""
    s = gpu.load()
    jobs = mixed_jobs()
    run_batch(s, jobs)
    run_batch(s, jobs, in_off=4, out_off=1)
    for op, data in jobs:
        assert s.luminance(data, op) == convert(op, data)
    assert s.luminance_batch([], V8) == ([], [])
    assert s.lib.spng_luminance_batch(s.ctx, None, 0, None, None) == 0


def test_results_on_the_device_and_on_the_host(gpu):
    """d_results alone (asynchronous), h_results alone, and both: the same results and the same pixels"""
    s = gpu.load()
    jobs = mixed_jobs()
    ins, outs, host, want = layout(jobs, 0, 0)
    n, size = len(jobs), ctypes.sizeof(gpu.Result)
    d_in = s.to_device(host)
    expect = [(0, ol, il, 0) for (_, il), (_, ol) in zip(ins, outs)]
    for on_device, on_host in ((True, False), (False, True), (True, True)):
        d_out = s.to_device(np.full_like(want, 0xEE))
        descs = (gpu.LuminanceDesc * n)(*[gpu.LuminanceDesc(d_in.data_ptr() + ia if il else None, d_out.data_ptr() + oa if il else None, il // 4, op)
                                          for (op, _), (ia, il), (oa, _) in zip(jobs, ins, outs)])
        d_res = s.to_device(np.full(n * size, 0xEE, dtype=np.uint8))
        h_res = (gpu.Result * n)()
        assert s.lib.spng_luminance_batch(s.ctx, descs, n, s._ptr(d_res) if on_device else None, h_res if on_host else None) == 0
        s.sync()
        assert np.array_equal(d_out.cpu().numpy(), want)
        if on_device:
            got = (gpu.Result * n).from_buffer_copy(d_res.cpu().numpy().tobytes())
            assert [(r.status, r.written, r.consumed, r.aux[0]) for r in got] == expect
        else:
            assert (d_res.cpu().numpy() == 0xEE).all()
        if on_host:
            assert [(r.status, r.written, r.consumed, r.aux[0]) for r in h_res] == expect


def test_refusals_leave_the_outputs_alone(gpu):
    """SPNG_E_ARGUMENT: a non-zero reserved byte, an unknown op, a null pointer with a non-zero count, d_out == d_in, any other
    overlap, a count whose byte size overflows; any alignment is accepted; nothing is enqueued by a refused call, not even for the
    valid descs in front of the spoiled one"""
    s = gpu.load()
    buf = s.to_device(np.full(8192, 0xEE, dtype=np.uint8))
    base = buf.data_ptr()
    assert base % 16 == 0

    def call(*descs):
        arr = (gpu.LuminanceDesc * len(descs))(*descs)
        res = (gpu.Result * len(descs))()
        return s.lib.spng_luminance_batch(s.ctx, arr, len(descs), None, res)

    def desc(d_in=base, d_out=base + 4096, count=16, op=V8, reserved=None):
        d = gpu.LuminanceDesc(d_in, d_out, count, op)
        if reserved is not None:
            d.reserved[reserved] = 1
        return d

    E = gpu.E_ARGUMENT
    spoiled = [desc(op=0), desc(op=3), desc(op=255)] + [desc(reserved=k) for k in range(7)]
    spoiled += [desc(d_in=None), desc(d_out=None), desc(d_in=None, d_out=None)]
    spoiled += [desc(d_out=base), desc(d_out=base, op=VA8), desc(d_out=base, count=0)]              # in place
    spoiled += [desc(d_out=base + 63), desc(d_out=base + 1), desc(d_in=base + 4096 + 15, d_out=base + 4096),
                desc(d_in=base + 4096 + 31, d_out=base + 4096, op=VA8)]                              # (16 pixels: 64 in, 16 or 32 out)
    spoiled += [desc(count=1 << 60), desc(count=(1 << 64) - 1, op=VA8), desc(count=(1 << 62) + 4)]
    for d in spoiled:
        assert call(d) == E
        assert call(desc(), d) == E and call(d, desc()) == E
    arr = (gpu.LuminanceDesc * 1)(desc())
    assert s.lib.spng_luminance_batch(s.ctx, arr, 1, None, None) == E                 # nowhere to put the results
    assert s.lib.spng_luminance_batch(None, arr, 1, None, (gpu.Result * 1)()) == E
    assert s.lib.spng_luminance_batch(s.ctx, None, 1, None, (gpu.Result * 1)()) == E
    res = gpu.Result()
    assert s.lib.spng_luminance(s.ctx, None, 4, V8, None, ctypes.byref(res)) == E
    assert s.lib.spng_luminance(s.ctx, None, 0, 3, None, ctypes.byref(res)) == E and s.lib.spng_luminance(s.ctx, None, 0, 0, None, ctypes.byref(res)) == E
    for pixels, op in ((b"\0" * 7, V8), (b"\0" * 8, 0), (b"\0" * 8, 3)):
        with pytest.raises(ValueError):
            s.luminance(pixels, op)
    s.sync()
    assert (buf.cpu().numpy() == 0xEE).all()
    # what is accepted: neighbours that touch, any alignment, empty descs with or without pointers, an empty call
    assert call(desc(d_out=base + 64)) == 0 and call(desc(d_in=base + 4096 + 16, d_out=base + 4096)) == 0
    assert call(desc(d_in=base + 4096 + 32, d_out=base + 4096, op=VA8)) == 0
    assert call(desc(d_in=base + 1, d_out=base + 4096 + 3)) == 0 and call(desc(d_in=base + 2, d_out=base + 4096 + 1, op=VA8)) == 0
    assert call(desc(count=0, d_in=None, d_out=None)) == 0 and call(desc(count=0)) == 0
    assert s.luminance(b"", V8) == b"" and s.luminance(b"", VA8) == b""


def test_the_kernel_is_timed_under_its_own_id(gpu):
    """SPNG_K_LUMINANCE = 19 lies inside SPNG_K_COUNT = 20: one launch is counted there, and 20 is no kernel"""
    s = gpu.load()
    d_in = s.to_device(np.zeros(4 * 64, dtype=np.uint8))
    s.profile(True)
    s.luminance_batch([d_in], V8)
    ms, launches = s.profile_get(gpu.K_LUMINANCE)
    s.profile(False)
    assert gpu.K_LUMINANCE == 19 and launches == 1 and ms >= 0
    assert s.lib.spng_profile_get(s.ctx, 20, ctypes.byref(ctypes.c_double(0)), ctypes.byref(ctypes.c_uint64(0))) == gpu.E_ARGUMENT


def test_mirror_luminance(gpu):
    rng = np.random.default_rng(5)
    px = rng.integers(0, 256, (1001, 4), dtype=np.uint8)
    want = tr.luminance(px)
    assert np.array_equal(gpu.PNG.luminance(px), want) and gpu.PNG.luminance(px.tobytes()) == want.tobytes()
    va = gpu.PNG.luminance(px, alpha=True)
    assert va.shape == (1001, 2) and np.array_equal(va[:, 0], want) and np.array_equal(va[:, 1], px[:, 3])
    with pytest.raises(ValueError):
        gpu.PNG.luminance(px.astype(np.uint16))
