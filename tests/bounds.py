"""Guard bytes around every source and destination of a stream call on the device (tests/test_gpu_bounds.py).

All sources of a call lie in ONE device tensor, all destinations in another; every buffer has GUARD bytes of 0xEE on both sides and
begins at a chosen residue 0 ... 15 from a 16-byte boundary.  The stream descriptors are built here, from pointers into the two
tensors.  Because every buffer lies deep inside an allocation the test owns, an overrun lands in guard bytes and is reported by
check(): nothing here can touch memory that is not the test's.  The sources must come back unchanged as well."""
from __future__ import annotations

import ctypes

import numpy as np

import swift_png_amd as spng

GUARD, FILL = 65536, 0xEE


class Arena:
    """srcs: bytes per stream (the same bytes object given twice is laid down once); caps: destination capacity per stream;
    src_res / dst_res: a residue for all, or one per stream.  dst_bytes: room laid out per destination where it is more than the
    capacity of a call (a destination used for several capacities)."""

    def __init__(self, s, srcs, caps, src_res=0, dst_res=0, dst_bytes=None):
        t = s.torch
        self.s, self.n = s, len(srcs)
        self.caps = [int(c) for c in caps]
        room = [int(c) for c in (dst_bytes if dst_bytes is not None else caps)]
        self.src_len = [len(b) for b in srcs]
        at, seen, self.src_off = GUARD, {}, []
        for i, b in enumerate(srcs):
            r = spng.pick(src_res, i)
            if (id(b), r) not in seen:
                off = (at + 15) // 16 * 16 + r
                seen[id(b), r] = off
                at = off + len(b) + GUARD
            self.src_off.append(seen[id(b), r])
        host = np.full(at + 16, FILL, np.uint8)
        for off, b in zip(self.src_off, srcs):
            host[off:off + len(b)] = np.frombuffer(b, np.uint8)
        self.src_host = host
        self.d_src = t.from_numpy(host.copy()).to(s.tdev)
        at, self.dst_off = GUARD, []
        for i, c in enumerate(room):
            off = (at + 15) // 16 * 16 + spng.pick(dst_res, i)
            self.dst_off.append(off)
            at = off + c + GUARD
        self.dst_total = at + 16
        self.d_dst = t.full((self.dst_total,), FILL, dtype=t.uint8, device=s.tdev)
        assert self.d_src.data_ptr() % 16 == 0 and self.d_dst.data_ptr() % 16 == 0
        self.used = self.caps

    def descs(self, fmts, reserved=0, src_len=None, caps=None):
        caps = self.caps if caps is None else [int(c) for c in caps]
        arr = (spng.StreamDesc * self.n)()
        for i in range(self.n):
            n = self.src_len[i] if src_len is None else int(spng.pick(src_len, i))
            assert n <= self.src_len[i]
            arr[i] = spng.StreamDesc(self.d_src.data_ptr() + self.src_off[i], n, self.d_dst.data_ptr() + self.dst_off[i], caps[i],
                                     int(spng.pick(fmts, i)), int(spng.pick(reserved, i)))
        self.used = caps
        return arr

    def preset(self, i, data):
        """bytes a destination holds before the call"""
        t = self.s.torch
        if len(data):
            self.d_dst[self.dst_off[i]:self.dst_off[i] + len(data)] = t.frombuffer(bytearray(data), dtype=t.uint8).to(self.s.tdev)

    def check(self, where=""):
        """every byte outside the destinations' [0, capacity) still 0xEE, the sources as they were; the first changed offset is named,
        relative to the stream it is nearest to.  -> the destinations' first `capacity` bytes"""
        host = self.d_dst.cpu().numpy()
        mask = np.ones(len(host), bool)
        for off, c in zip(self.dst_off, self.used):
            mask[off:off + c] = False
        bad = np.nonzero(mask & (host != FILL))[0]
        if len(bad):
            p = int(bad[0])
            i = max((k for k in range(self.n) if self.dst_off[k] <= p), key=lambda k: self.dst_off[k], default=-1)
            if i >= 0 and (p < self.dst_off[i] + self.used[i] + GUARD or i + 1 >= self.n):
                what = "destination %d (capacity %d, residue %d): byte %d behind its capacity" % (
                    i, self.used[i], self.dst_off[i] % 16, p - self.dst_off[i] - self.used[i])
            else:
                what = "destination %d (residue %d): byte %d in front of it" % (i + 1, self.dst_off[i + 1] % 16, self.dst_off[i + 1] - p)
            raise AssertionError("%s: guard byte changed, %s; %d guard bytes changed in all" % (where, what, len(bad)))
        src = self.d_src.cpu().numpy()
        diff = np.nonzero(src != self.src_host)[0]
        assert not len(diff), "%s: source bytes changed, first at %d" % (where, int(diff[0]))
        return [host[off:off + c].tobytes() for off, c in zip(self.dst_off, self.used)]


def inflate(s, srcs, caps, fmts, src_res=0, dst_res=0, where=""):
    """spng_inflate_batch between guards -> [(Result, the destination's first `capacity` bytes)]"""
    a = Arena(s, srcs, caps, src_res, dst_res)
    res = (spng.Result * a.n)()
    spng._check(s.lib, s.lib.spng_inflate_batch(s.ctx, a.descs(fmts), a.n, None, res))
    return list(zip(list(res), a.check(where)))


def deflate(s, srcs, caps, fmts, levels, exponents=0, src_res=0, dst_res=0, where=""):
    """spng_deflate_batch between guards -> [(Result, the destination's first `capacity` bytes)]"""
    a = Arena(s, srcs, caps, src_res, dst_res)
    lv = (ctypes.c_int32 * a.n)(*[int(spng.pick(levels, i)) for i in range(a.n)])
    res = (spng.Result * a.n)()
    spng._check(s.lib, s.lib.spng_deflate_batch(s.ctx, a.descs(fmts, exponents), lv, a.n, None, res))
    return list(zip(list(res), a.check(where)))


class InflatePush:
    """one stream through spng_inflate_resume_batch between guards: push(src_len) -> (Result, the destination's bytes)"""

    def __init__(self, s, z, cap, fmt):
        self.s, self.a, self.fmt, self.state = s, Arena(s, [z], [cap]), fmt, (0, 0, 0, 0)

    def push(self, src_len, where=""):
        s = self.s
        st = (ctypes.c_uint64 * 4)(*self.state)
        res = (spng.Result * 1)()
        spng._check(s.lib, s.lib.spng_inflate_resume_batch(s.ctx, self.a.descs(self.fmt, src_len=src_len), st, 1, None, res))
        r = res[0]
        if r.status == spng.NEED_MORE_INPUT:                                     # (Session.inflate_resume: the four words of state)
            tok = int(r.consumed)
            self.state = (int(r.aux[0]), int(r.aux[1]), tok, int(r.written) if tok else 0)
        return r, self.a.check(where)[0]


class DeflatePush:
    """one stream through spng_deflate_resume_batch between guards: push(src_len, last) -> (Result, the destination's bytes)"""

    def __init__(self, s, data, cap, fmt, level, exponent=0):
        t = s.torch
        self.s, self.a, self.fmt, self.level, self.exponent = s, Arena(s, [data], [cap]), fmt, level, exponent
        self.state = t.zeros(int(s.lib.spng_deflate_state_bytes()), dtype=t.uint8, device=s.tdev)
        self.hstate = (0, 0)

    def push(self, src_len, last, where=""):
        s = self.s
        lv = (ctypes.c_int32 * 1)(self.level)
        st = (ctypes.c_void_p * 1)(self.state.data_ptr())
        la = (ctypes.c_uint8 * 1)(1 if last else 0)
        hs = (ctypes.c_uint64 * 2)(*self.hstate)
        res = (spng.Result * 1)()
        spng._check(s.lib, s.lib.spng_deflate_resume_batch(s.ctx, self.a.descs(self.fmt, self.exponent, src_len=src_len), lv, st, la, hs, 1, None, res))
        r = res[0]
        self.hstate = (int(r.aux[0]), int(r.aux[1]))
        return r, self.a.check(where)[0]
