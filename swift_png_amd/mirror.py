"""Python mirror of the reference's own API for the hot path, delegating to the C ABI.

Names, argument meaning and error behaviour follow the Swift originals so that the parity tests
read like the reference's tests.  State that the reference keeps as a resumable state machine
(LZ77.InflatorState, PNG.Decoder.row/pass) is kept on the device between pushes: the compressed bytes and the
inflated bytes so far, and the point (a block boundary) from which the next push goes on
(spng_inflate_resume_batch).
"""
from __future__ import annotations

import struct

from . import (DONE, FORMAT_GZIP, FORMAT_IOS, FORMAT_ZLIB, NEED_MORE_INPUT, DecodingError, SpngError,
               E_EXTRANEOUS_COMPRESSED_DATA, E_INCOMPLETE_DATASTREAM, E_OUTPUT_CAPACITY, IMAGE_OVERDRAW,
               HSVA_FROM_RGBA8, HSVA_TO_RGBA8, HSVA_TO_VA8, LUMINANCE_V8, LUMINANCE_VA8, PREMULTIPLY, PREMULTIPLY_AS_U8, STRAIGHTEN, STRAIGHTEN_AS_U8, TARGET_RGBA,
               TARGET_VA)

_DELAY_FORMATS = {1: (8, 1), 2: (8, 2), 3: (8, 3), 4: (8, 4), 6: (16, 3), 8: (16, 4)}


class ChunkOrderError(Exception):
    """The cases of PNG.DecodingError about which chunks a file holds and in which order: the host's business"""


class RequiredChunk(ChunkOrderError):
    """PNG.DecodingError.required(chunk:before:)"""

    def __init__(self, chunk, before):
        self.chunk, self.before = chunk, before
        super().__init__(f"required({chunk}, before: {before})")


class DuplicateChunk(ChunkOrderError):
    """PNG.DecodingError.duplicate(chunk:)"""

    def __init__(self, chunk):
        self.chunk = chunk
        super().__init__(f"duplicate({chunk})")


class UnexpectedChunk(ChunkOrderError):
    """PNG.DecodingError.unexpected(chunk:after:)"""

    def __init__(self, chunk, after):
        self.chunk, self.after = chunk, after
        super().__init__(f"unexpected({chunk}, after: {after})")


def _name(type_code: int) -> str:
    return struct.pack(">I", type_code).decode("latin-1")


_BEFORE_PLTE = ("cHRM", "gAMA", "sRGB", "iCCP", "sBIT")
# the fields of PNG.Metadata by chunk type: (attribute, typed)
_UNIQUE = {"cHRM": "chromaticity", "gAMA": "gamma", "sRGB": "colorRendering", "iCCP": "colorProfile", "sBIT": "significantBits",
           "hIST": "histogram", "pHYs": "physicalDimensions", "tIME": "time"}


class Text:
    """PNG.Text (Sources/PNG/Parsing/PNG.Text.swift:6-99): compressed, keyword (english, localized), language, content"""

    def __init__(self, compressed, keyword, language, content):
        self.compressed, self.keyword, self.language, self.content = bool(compressed), tuple(keyword), list(language), content

    def __eq__(self, other):
        return isinstance(other, Text) and vars(self) == vars(other)

    def __repr__(self):
        return f"Text(compressed={self.compressed}, keyword={self.keyword}, language={self.language}, content=<{len(self.content)} characters>)"

    def head(self) -> bytes:
        """`serialized` up to the content (:317-332)"""
        english, localized = self.keyword
        return (english.encode("latin-1") + b"\0" + bytes([1 if self.compressed else 0, 0]) +
                b"-".join(t.encode("latin-1") for t in self.language) + b"\0" +
                (localized.encode("utf-8") if localized != english else b"") + b"\0")


class ColorProfile:
    """PNG.ColorProfile (Sources/PNG/Parsing/PNG.ColorProfile.swift:5-44): name, profile"""

    def __init__(self, name, profile):
        self.name, self.profile = name, bytes(profile)

    def __eq__(self, other):
        return isinstance(other, ColorProfile) and vars(self) == vars(other)


class Metadata:
    """PNG.Metadata (Sources/PNG/Decoding/PNG.Metadata.swift:5-95).  Typed: time -- (year, month, day, hour, minute, second),
    PNG.TimeModified --, gamma -- the numerator over 100000, PNG.Gamma --, physicalDimensions -- (x, y, unit byte),
    PNG.PhysicalDimensions --, colorProfile -- ColorProfile --, text -- [Text].  From PNG.decompress(typed=True), out of the records of
    spng_parse_dir_batch: chromaticity -- the eight values in payload order, PNG.Chromaticity --, colorRendering -- the code,
    PNG.ColorRendering --, significantBits -- the precisions, PNG.SignificantBits --, histogram -- the frequencies, PNG.Histogram --,
    suggestedPalettes -- (name, depth, [(r, g, b, a, frequency)]), PNG.SuggestedPalette.  From the default, untyped decompress these
    five are carried as their payload bytes, uninterpreted (a field that holds bytes is written back as it is).  application: a list
    of (type, payload)."""

    def __init__(self, time=None, chromaticity=None, colorProfile=None, colorRendering=None, gamma=None, histogram=None,
                 physicalDimensions=None, significantBits=None, suggestedPalettes=(), text=(), application=()):
        self.time, self.chromaticity, self.colorProfile, self.colorRendering = time, chromaticity, colorProfile, colorRendering
        self.gamma, self.histogram, self.physicalDimensions, self.significantBits = gamma, histogram, physicalDimensions, significantBits
        self.suggestedPalettes, self.text, self.application = list(suggestedPalettes), list(text), list(application)

    def push(self, chunk, palette_seen=False, parsed=None, value=None):
        """push(ancillary:pixel:palette:background:transparency:) (PNG.Metadata.swift:151-245) for every chunk but bKGD and tRNS,
        which are the format's: chunk = (type, payload); parsed: the Text or ColorProfile of a text or profile chunk, which the
        device has taken apart (PNG.decompress).  Raises UnexpectedChunk for cHRM gAMA sRGB iCCP sBIT behind PLTE (:159-164),
        RequiredChunk for hIST without PLTE (:190-194), DuplicateChunk for a second one of the unique chunks (:98-108).  value: the
        chunk's record of spng_parse_dir_batch; with one, its status is raised behind those rules -- unique(assign:) looks for the
        duplicate before it parses (:99-108) -- and the field is typed from it."""
        from . import ParsingError
        kind, payload = chunk
        if kind in ("CgBI", "IHDR", "PLTE", "IDAT", "IEND", "bKGD", "tRNS"):
            raise ValueError(f"Metadata.push cannot be used with chunk type '{kind}'")       # (:166-170: fatalError)
        if kind in _BEFORE_PLTE and palette_seen:
            raise UnexpectedChunk(kind, "PLTE")
        if kind == "hIST" and not palette_seen:
            raise RequiredChunk("PLTE", "hIST")
        if kind in _UNIQUE:
            if getattr(self, _UNIQUE[kind]) is not None:
                raise DuplicateChunk(kind)
            if value is not None and value.status != DONE:
                raise ParsingError(value.status, tuple(value.aux))
            if value is not None and kind != "iCCP":             # the record's words, as many as the field has
                v, count = tuple(value.v), value.count
                if kind == "hIST":
                    value = list(struct.unpack(">" + "H" * count, payload))
                else:
                    width = {"gAMA": 1, "sRGB": 1, "pHYs": 3, "tIME": 6, "cHRM": 8, "sBIT": len(payload)}[kind]
                    value = v[0] if width == 1 and kind != "sBIT" else v[:width]
            elif kind == "gAMA":                                  # PNG.Gamma.init(parsing:): one big-endian UInt32
                value = struct.unpack(">I", payload)[0]
            elif kind == "pHYs":                                 # PNG.PhysicalDimensions.init(parsing:): x, y, unit
                value = struct.unpack(">IIB", payload)
            elif kind == "tIME":                                 # PNG.TimeModified.init(parsing:)
                value = struct.unpack(">HBBBBB", payload)
            elif kind == "iCCP":
                value = parsed
            else:
                value = bytes(payload)
            setattr(self, _UNIQUE[kind], value)
        elif kind == "sPLT":
            if value is not None and value.status != DONE:
                raise ParsingError(value.status, tuple(value.aux))
            if value is not None:                                # PNG.SuggestedPalette.swift:79-112
                fmt = ">BBBBH" if value.v[0] == 8 else ">HHHHH"
                entries = [struct.unpack_from(fmt, payload, value.k + 2 + i * struct.calcsize(fmt)) for i in range(value.count)]
                self.suggestedPalettes.append((payload[:value.k].decode("latin-1"), value.v[0], entries))
            else:
                self.suggestedPalettes.append(bytes(payload))
        elif kind in ("iTXt", "tEXt", "zTXt"):
            self.text.append(parsed)
        else:
            self.application.append((kind, bytes(payload)))

    def chunks(self, deflated):
        """-> (before, after): the chunks PNG.Image.compress writes in front of PLTE and behind tRNS, in its order
        (PNG.Image.swift:596-656).  deflated: the streams of colorProfile and of the compressed texts, in that order"""
        deflated = list(deflated)
        before, after = [], []
        raw = lambda v, pack: bytes(v) if isinstance(v, (bytes, bytearray)) else pack(v)  # noqa: E731  (an untyped field: as it came)

        def palette(p):                                          # PNG.SuggestedPalette.serialized
            name, depth, entries = p
            return name.encode("latin-1") + b"\0" + bytes([depth]) + b"".join(struct.pack(">BBBBH" if depth == 8 else ">HHHHH", *e) for e in entries)
        if self.chromaticity is not None:
            before.append(("cHRM", raw(self.chromaticity, lambda v: struct.pack(">8I", *v))))
        if self.gamma is not None:
            before.append(("gAMA", struct.pack(">I", self.gamma)))
        if self.colorRendering is not None:
            before.append(("sRGB", raw(self.colorRendering, lambda v: bytes([v]))))
        if self.colorProfile is not None:                        # PNG.ColorProfile.serialized (PNG.ColorProfile.swift:87-103)
            before.append(("iCCP", self.colorProfile.name.encode("latin-1") + b"\0\0" + deflated.pop(0)))
        if self.significantBits is not None:
            before.append(("sBIT", raw(self.significantBits, bytes)))
        if self.histogram is not None:
            after.append(("hIST", raw(self.histogram, lambda v: struct.pack(">" + "H" * len(v), *v))))
        if self.physicalDimensions is not None:
            after.append(("pHYs", struct.pack(">IIB", *self.physicalDimensions)))
        if self.time is not None:
            after.append(("tIME", struct.pack(">HBBBBB", *self.time)))
        for t in self.text:                                      # every text as iTXt (PNG.Text.serialized, PNG.Text.swift:309-349)
            after.append(("iTXt", t.head() + (deflated.pop(0) if t.compressed else t.content.encode("utf-8"))))
        after += [("sPLT", raw(p, palette)) for p in self.suggestedPalettes] + list(self.application)
        as_bytes = lambda cs: [(k.encode("latin-1") if isinstance(k, str) else bytes(k), bytes(p)) for k, p in cs]  # noqa: E731
        return as_bytes(before), as_bytes(after)

    def to_deflate(self):
        """what `chunks` wants deflated at level 13, exponent 15: the profile, the contents of the compressed texts"""
        return ([self.colorProfile.profile] if self.colorProfile is not None else []) + [t.content.encode("utf-8") for t in self.text if t.compressed]


class Image:
    """What PNG.decompress returns: size, the pieces of the format as PNG.compress takes them, storage, metadata"""

    def __init__(self, size, depth, channels, indexed, bgr, interlaced, palette, key, fill, storage, metadata):
        self.size, self.depth, self.channels, self.indexed, self.bgr, self.interlaced = size, depth, channels, indexed, bgr, interlaced
        self.palette, self.key, self.fill, self.storage, self.metadata = palette, key, fill, storage, metadata

    def format(self) -> dict:
        return dict(indexed=self.indexed, bgr=self.bgr, interlaced=self.interlaced, palette=self.palette, key=self.key, fill=self.fill)


class LZ77:
    class Format:
        zlib = FORMAT_ZLIB
        ios = FORMAT_IOS

    class Inflator:
        """LZ77.Inflator (Sources/LZ77/Inflator/LZ77.Inflator.swift:8-62).

        Streaming like the original: the compressed bytes pushed so far and the bytes inflated so far stay on the
        device, and a push goes on where the previous one stopped (spng_inflate_resume_batch: blocks the input now
        holds completely are decoded once, by the parallel pipeline; only the block the input ends in is decoded
        again by the next push).  gzip members (Gzip.Inflator) too: their few header bytes are parsed again by every
        push (LZ77.InflatorBuffers.swift:139-230), their DEFLATE payload is not."""

        def __init__(self, format=FORMAT_ZLIB, session=None):
            from . import load
            self._s = session or load()
            self._format = format
            self._streaming = True
            self._in = bytearray()
            self._d_in, self._n_in = None, 0      # device: all compressed bytes so far
            self._d_out = None                    # device: all inflated bytes so far
            self._state = (0, 0, 0, 0)
            self._out = b""
            self._avail = 0
            self._cursor = 0
            self._terminal = False

        def _append(self, data):
            s, t = self._s, self._s.torch
            need = self._n_in + len(data)
            if self._d_in is None or self._d_in.numel() < need:
                grown = s.empty(max(2 * need, 1 << 16))
                if self._n_in:
                    grown[:self._n_in] = self._d_in[:self._n_in]
                self._d_in = grown
            if data:
                self._d_in[self._n_in:need] = s.to_device(bytes(data))
            self._n_in = need

        def push(self, data) -> object:
            """Returns None once a complete stream has been received, () while it wants more."""
            from . import raise_for
            if self._terminal:
                return None                      # .terminal: remaining input is ignored (:38-40)
            if not self._streaming:
                self._in += bytes(data)
                cap = max(1 << 16, 1100 * len(self._in))
                while True:
                    status, out, _, aux = self._s.inflate(bytes(self._in), self._format, cap)
                    if status != E_OUTPUT_CAPACITY:
                        break
                    cap *= 4                     # the reference's output buffer is unbounded
                raise_for(status, aux)
                self._out, self._avail = out, len(out)
                self._terminal = status == DONE
                return None if self._terminal else ()
            self._append(data)
            if self._d_out is None:
                self._d_out = self._s.empty(max(1 << 16, 8 * self._n_in))
            while True:
                res, state = self._s.inflate_resume(self._d_in, self._n_in, self._d_out, self._format, self._state)
                if res.status != E_OUTPUT_CAPACITY:
                    break
                grown = self._s.empty(4 * self._d_out.numel())          # the reference's output buffer is unbounded
                grown[:self._d_out.numel()] = self._d_out
                self._d_out = grown
            raise_for(res.status, (res.aux[0], res.aux[1]))
            self._state, self._avail = state, res.written
            self._terminal = res.status == DONE
            return None if self._terminal else ()

        def _bytes(self, a, b):
            if not self._streaming:
                return self._out[a:b]
            return bytes(self._d_out[a:b].cpu().numpy()) if b > a else b""

        def pull(self, count=None):
            if count is None:                    # pull() -> everything available (:58-61)
                data, self._cursor = self._bytes(self._cursor, self._avail), self._avail
                return data
            if self._avail - self._cursor < count:
                return None                      # pull(_:) -> nil (:53-56)
            data = self._bytes(self._cursor, self._cursor + count)
            self._cursor += count
            return data


    class Deflator:
        """LZ77.Deflator (Sources/LZ77/Deflator/LZ77.Deflator.swift:8-44): init(format:level:exponent:hint:),
        push(_:last:), pull(), pop().  Every push goes to the device (spng_deflate_resume_batch): the input so far and the
        stream so far live in HBM, the compressor's state -- parse position, queued terms, symbol costs, block limit, bit
        writer -- in a device-side state block, and a push emits what the bytes so far determine (the reference compresses
        whenever more than 4096 bytes are buffered, LZ77.DeflatorBuffers.swift:68-93; its output does not depend on how the
        input was pushed, SURVEY 8a row a13, and neither does this one).  pop() hands out complete chunks of 2 * hint bytes
        (the reference's chunk is 2 * ManagedBuffer.capacity >= 2 * hint bytes, a platform-dependent size) and pull() also
        whatever has been written so far -- their concatenation is the reference's stream bit for bit.  One known difference,
        on a reference bug: a row-by-row pushed stream whose last non-final compress() leaves fewer than three bytes queued
        makes the reference emit a corrupt stored tail (DeflatorBuffers.Stream.swift:45-60); this class emits the correct
        stream instead."""

        def __init__(self, format=FORMAT_ZLIB, level=9, exponent=15, hint=1 << 12, session=None):
            from . import load
            if not 8 <= exponent <= 15:
                raise ValueError("exponent must be 8 ... 15")
            self._s = session or load()
            self._format, self._level, self._exponent = format, level, exponent
            self._chunk = 2 * max(int(hint), 1)
            s = self._s
            self._d_in, self._n = s.empty(1 << 16), 0
            self._d_out = s.empty(s.lib.spng_deflate_bound(1 << 16))
            self._state = s.torch.zeros(int(s.lib.spng_deflate_state_bytes()), dtype=s.torch.uint8, device=s.tdev)
            self._hstate = (0, 0)
            self._avail = 0                      # stream bytes the device has produced so far
            self._cursor = 0
            self._done = False
            self.device_calls = 0

        def push(self, data, last=False):
            if self._done:
                raise RuntimeError("push after the last block")
            s, data = self._s, bytes(data)
            need = self._n + len(data)
            if self._d_in.numel() < need:
                grown = s.empty(2 * need); grown[:self._n] = self._d_in[:self._n]; self._d_in = grown
            if data:
                self._d_in[self._n:need] = s.to_device(data)
            self._n = need
            cap = int(s.lib.spng_deflate_bound(need)) + 64
            if self._d_out.numel() < cap:
                grown = s.empty(2 * cap); grown[:self._avail + 8] = self._d_out[:self._avail + 8]; self._d_out = grown
            res, self._hstate = s.deflate_resume(self._d_in, self._n, self._d_out, self._level, self._state, last, self._format,
                                                 self._exponent, self._hstate)
            self.device_calls += 1
            if res.status not in (DONE, NEED_MORE_INPUT):
                raise SpngError(res.status)
            self._avail = res.written
            self._done = bool(last)

        def _bytes(self, a, b):
            return bytes(self._d_out[a:b].cpu().numpy()) if b > a else b""

        def pop(self):
            """A complete chunk, or None (:40-43)."""
            if self._avail - self._cursor < self._chunk:
                return None
            data = self._bytes(self._cursor, self._cursor + self._chunk)
            self._cursor += self._chunk
            return data

        def pull(self):
            """A complete chunk if there is one, else whatever has been written so far, else None (:31-35)."""
            data = self.pop()
            if data is not None:
                return data
            if self._cursor >= self._avail:
                return None
            data, self._cursor = self._bytes(self._cursor, self._avail), self._avail
            return data


class Gzip:
    """Gzip (Sources/LZ77/Gzip/Gzip.swift:1-47): the LZ77 codec behind a gzip member -- header with FEXTRA / FNAME /
    FCOMMENT skipped, CRC-32 checked, ISIZE read (Gzip.StreamHeader.swift:17-97, LZ77.InflatorBuffers.swift:139-230);
    on the way out the fixed ten-byte header and the CRC-32 / byte-count trailer (LZ77.DeflatorBuffers.swift:96-135)."""

    class Inflator(LZ77.Inflator):
        """Gzip.Inflator (Gzip.Inflator.swift:1-58): init(), push(_:), pull(_:), pull()."""

        def __init__(self, session=None):
            super().__init__(FORMAT_GZIP, session)

    class Deflator(LZ77.Deflator):
        """Gzip.Deflator (Gzip.Deflator.swift:1-40): init(level:exponent:hint:), push(_:last:), pull(), pop()."""

        def __init__(self, level, exponent=15, hint=1 << 12, session=None):
            super().__init__(FORMAT_GZIP, level, exponent, hint, session)

    @staticmethod
    def extract(data, session=None) -> bytes:
        """Gzip.extract(from:) (Gzip.swift:5-11)"""
        inflator = Gzip.Inflator(session)
        inflator.push(data)
        return inflator.pull()

    @staticmethod
    def archive(data, level=7, hint=128 << 10, session=None) -> bytes:
        """Gzip.archive(bytes:level:hint:) (Gzip.swift:32-46)"""
        deflator = Gzip.Deflator(level, hint=hint, session=session)
        deflator.push(data, last=True)
        out = b""
        while (part := deflator.pull()) is not None:
            out += part
        return out


def _alpha(layout, pixels, bits, op, session):
    """an array of RGBA<T> / VA<T> pixels (numpy array of T, or bytes in host order) through spng_alpha: -> (the same kind of
    object, components the reference would have trapped on)"""
    from . import load
    s = session or load()
    if isinstance(pixels, (bytes, bytearray, memoryview)):
        return s.alpha(bytes(pixels), bits, layout, op)
    import numpy as np
    a = np.ascontiguousarray(pixels)
    if a.dtype.itemsize * 8 != bits or a.dtype.kind != "u":
        raise ValueError("the array's element type must be the unsigned integer of `bits` bits")
    out, trapped = s.alpha(a.tobytes(), bits, layout, op)
    return np.frombuffer(out, dtype=a.dtype).reshape(a.shape).copy(), trapped


class _ColorTarget:
    """premultiplied / straightened of a colour target mapped over an array of pixels, on the device"""
    _layout = TARGET_RGBA

    @classmethod
    def premultiplied(cls, pixels, bits, as_u8=False, session=None):
        """.premultiplied / .premultiplied(as: UInt8.self) (PNG.RGBA.swift:121-158, PNG.VA.swift:57-87)"""
        return _alpha(cls._layout, pixels, bits, PREMULTIPLY_AS_U8 if as_u8 else PREMULTIPLY, session)[0]

    @classmethod
    def straightened(cls, pixels, bits, as_u8=False, session=None):
        """.straightened / .straightened(as: UInt8.self) (PNG.RGBA.swift:167-206, PNG.VA.swift:98-131).  Where the reference
        traps -- a colour above its alpha: the quotient does not fit T -- this raises ValueError."""
        out, trapped = _alpha(cls._layout, pixels, bits, STRAIGHTEN_AS_U8 if as_u8 else STRAIGHTEN, session)
        if trapped:
            raise ValueError(f"{trapped} components exceed their alpha: not representable in T (the reference traps)")
        return out


def _hsva(pixels, op, session):
    """an array of pixels (bytes in host order, or a numpy array: (n, 4) uint8 going in, records of PNG.HSVA.dtype() coming out)
    through spng_hsva: -> (the converted array, bytes for bytes, pixels the reference would have trapped on)"""
    from . import load
    s = session or load()
    if isinstance(pixels, (bytes, bytearray, memoryview)):
        return s.hsva(bytes(pixels), op)
    import numpy as np
    a = np.ascontiguousarray(pixels)
    if a.dtype != (np.dtype(np.uint8) if op == HSVA_FROM_RGBA8 else PNG.HSVA.dtype()):
        raise ValueError("uint8 components going in, records of PNG.HSVA.dtype() coming out")
    out, trapped = s.hsva(a.tobytes(), op)
    if op == HSVA_FROM_RGBA8:
        return np.frombuffer(out, dtype=PNG.HSVA.dtype()).copy(), trapped
    return np.frombuffer(out, dtype=np.uint8).reshape(-1, 4 if op == HSVA_TO_RGBA8 else 2).copy(), trapped


class PNG:
    @staticmethod
    def luminance(pixels, alpha=False, session=None):
        """rgba.map(COMPUTE_LUMINANCE) of the reference's tutorial (Snippets/PNG/BasicEncoding.swift:63-71) on the device: RGBA<UInt8>
        pixels as bytes or as an (n, 4) uint8 numpy array -> the [UInt8] the tutorial packs (bytes for bytes, an (n,) array for an
        array); alpha=True: (l, a) pairs, an (n, 2) array"""
        from . import load
        s = session or load()
        op = LUMINANCE_VA8 if alpha else LUMINANCE_V8
        if isinstance(pixels, (bytes, bytearray, memoryview)):
            return s.luminance(bytes(pixels), op)
        import numpy as np
        a = np.ascontiguousarray(pixels)
        if a.dtype != np.uint8:
            raise ValueError("uint8 components are needed")
        out = np.frombuffer(s.luminance(a.tobytes(), op), dtype=np.uint8)
        return out.reshape(-1, 2).copy() if alpha else out.copy()

    class HSVA:
        """The custom colour target of the reference's tutorial (Snippets/PNG/CustomColor.swift: struct HSVA { h: UInt32, s: UInt16,
        v: UInt8, a: UInt8 }, PNG.Color conformance :82-301) on the device: arrays of 8-byte records, host byte order."""

        @staticmethod
        def dtype():
            import numpy as np
            return np.dtype([("h", "<u4"), ("s", "<u2"), ("v", "u1"), ("a", "u1")])

        @staticmethod
        def from_rgba(pixels, session=None):
            """[PNG.RGBA<UInt8>].map{ HSVA.init(r: $0.r, g: $0.g, b: $0.b, a: $0.a) } (CustomColor.swift:19-49)"""
            return _hsva(pixels, HSVA_FROM_RGBA8, session)[0]

        @staticmethod
        def rgba(pixels, session=None):
            """[HSVA].map(\\.rgba) (CustomColor.swift:51-78).  Where the reference traps -- fatalError("unreachable"): h of 6 * 65537
            or more in a pixel with s > 0 and v > 0 -- this raises ValueError."""
            out, trapped = _hsva(pixels, HSVA_TO_RGBA8, session)
            if trapped:
                raise ValueError(f"{trapped} pixels have a hue of 6 * 65537 or more: unreachable (the reference traps)")
            return out

        @staticmethod
        def va(pixels, session=None):
            """the (v, a) of every pixel: what HSVA.pack stores for the grey formats (CustomColor.swift:232-251)"""
            return _hsva(pixels, HSVA_TO_VA8, session)[0]

        @staticmethod
        def unpack(storage: bytes, w, h, depth, channels, indexed=False, bgr=False, palette=None, key=None, deindexer=None,
                   session=None) -> bytes:
            """PNG.Image.unpack(as: HSVA.self) (HSVA.unpack, CustomColor.swift:86-210): Session.unpack's arguments without the
            target's own (target, layout, premultiply).  Two steps on the device: RGBA<UInt8>.unpack, then HSVA.init(r:g:b:a:) -- for
            every format what the tutorial's switch computes (include/spng_mi355.h).  -> bytes of HSVA records"""
            from . import load
            s = session or load()
            rgba = s.unpack(storage, w, h, depth, channels, indexed=indexed, bgr=bgr, target=8, palette=palette, key=key,
                            layout=TARGET_RGBA, deindexer=deindexer)
            return s.hsva(rgba, HSVA_FROM_RGBA8)[0]

        @staticmethod
        def pack(pixels: bytes, w, h, depth, channels, indexed=False, bgr=False, palette=None, indexer=None, session=None) -> bytes:
            """PNG.Image(packing: [HSVA], size:layout:).storage (HSVA.pack, CustomColor.swift:213-299): Session.pack's arguments
            without the source's own (source, layout, premultiply).  Grey formats store (v, a) (kernel: \\.v): HSVA_TO_VA8, then the
            VA<UInt8> pack; colour and indexed formats store .rgba: HSVA_TO_RGBA8, then the RGBA<UInt8> pack with the default or
            the given indexer.  ValueError where .rgba traps."""
            from . import load
            s = session or load()
            if len(pixels) != 8 * w * h:
                raise ValueError("pixel array `count` must be equal to `size.x * size.y`")
            if not indexed and channels <= 2:
                return s.pack(s.hsva(bytes(pixels), HSVA_TO_VA8)[0], w, h, depth, channels, source=8, layout=TARGET_VA)
            return s.pack(PNG.HSVA.rgba(bytes(pixels), session=s), w, h, depth, channels, indexed=indexed, bgr=bgr, source=8,
                          palette=palette, layout=TARGET_RGBA, indexer=indexer)

    class Standard:
        common = FORMAT_ZLIB
        ios = FORMAT_IOS

    class RGBA(_ColorTarget):
        """PNG.RGBA<T> (Sources/PNG/ColorTargets/PNG.RGBA.swift): arrays of (r, g, b, a)"""
        _layout = TARGET_RGBA

    class VA(_ColorTarget):
        """PNG.VA<T> (Sources/PNG/ColorTargets/PNG.VA.swift): arrays of (v, a)"""
        _layout = TARGET_VA

    class Decoder:
        @staticmethod
        def defilter(line: bytes, last: bytes, delay: int, session=None) -> bytes:
            """PNG.Decoder.defilter(_:last:delay:) (PNG.Decoder.swift:152-196).  `line` and `last`
            are pitch+1 bytes (index 0 = filter byte).  delay must be a real PNG pixel stride
            (1, 2, 3, 4, 6 or 8)."""
            from . import load
            s = session or load()
            pitch = len(line) - 1
            depth, channels = _DELAY_FORMATS[delay]
            assert pitch % delay == 0
            rows = bytes([0]) + bytes(last[1:]) + bytes(line)
            _, storage = s.unfilter(rows, pitch // delay, 2, depth, channels, False)
            return bytes(line[:1]) + storage[pitch:]

    class Encoder:
        @staticmethod
        def filter(line: bytes, last: bytes, delay: int, session=None) -> bytes:
            """PNG.Encoder.filter(_:last:delay:) (PNG.Encoder.swift:132-204): line[0] == 0."""
            from . import load
            s = session or load()
            pitch = len(line) - 1
            depth, channels = _DELAY_FORMATS[delay]
            assert pitch % delay == 0
            rows = s.filter(bytes(last[1:]) + bytes(line[1:]), pitch // delay, 2, depth, channels, False)
            return rows[pitch + 1:]

    class ImageEncoder:
        """PNG.Encoder driven over a whole image (PNG.Encoder.pull, Sources/PNG/Encoding/PNG.Encoder.swift:33-129,
        as PNG.Image.compress(stream:level:hint:) loops over it, PNG.Image.swift:658-665): every pull returns the
        payload of the next IDAT chunk, None when the stream is exhausted.  Filter selection and DEFLATE run on the
        device in one spng_encode_batch call at the first pull."""

        def __init__(self, storage: bytes, size, depth, channels, interlaced=False, standard=FORMAT_ZLIB, level=9,
                     hint=1 << 15, session=None):
            from . import load
            self._s = session or load()
            self._args = (bytes(storage), size[0], size[1], depth, channels, bool(interlaced))
            self._standard, self._level = standard, level
            self._chunk = 2 * max(int(hint), 1)
            self._out, self._cursor = None, 0

        def pull(self):
            if self._out is None:
                rows = self._s.filter(*self._args)
                self._out = self._s.deflate(rows, self._level, self._standard)
            if self._cursor >= len(self._out):
                return None
            data = self._out[self._cursor:self._cursor + self._chunk]
            self._cursor += len(data)
            return data

    Metadata, Text, ColorProfile, Image = Metadata, Text, ColorProfile, Image

    @staticmethod
    def _walk(entries, names, info, metadata, work, payload, values=None):
        """the loops of PNG.Image.decompress behind IHDR (PNG.Image.swift:323-399) over a file's directory: which chunks may stand
        where.  Text and profile chunks go to `work`, their places to the metadata; PLTE, bKGD, tRNS to metadata._critical.  values: the
        records of spng_parse_dir_batch beside the entries (typed): a chunk's order rules come first, then its record's status; the
        records of PLTE, bKGD, tRNS go to metadata._records"""
        from . import SCOPE_NO_PALETTE, ParsingError
        plte = bkgd = trns = None
        seen_idat = done_idat = False
        metadata._critical = (None, None, None)
        metadata._records = {}

        def parsed(kind, v):
            if v is None:
                return
            if v.scope == SCOPE_NO_PALETTE:                      # PNG.Transparency.swift:165-169, PNG.Background.swift:158-162
                raise RequiredChunk("PLTE", kind)
            if v.status != DONE:
                raise ParsingError(v.status, tuple(v.aux))
            metadata._records[kind] = v
        for i, (e, kind) in enumerate(zip(entries, names)):
            value = values[i] if values is not None else None
            if kind == "IDAT":
                if done_idat:
                    raise UnexpectedChunk("IDAT", "IDAT")        # (PNG.Context.swift:133-135)
                if not seen_idat and info.color == 3 and plte is None:
                    raise RequiredChunk("PLTE", "IDAT")          # :363-365
                seen_idat = True
                continue
            done_idat = seen_idat
            if kind == "IEND":
                if not seen_idat:
                    raise RequiredChunk("IDAT", "IEND")          # :368-369
                break
            if seen_idat:                                        # PNG.Context.push(ancillary:) (PNG.Context.swift:120-146)
                if kind in ("CgBI", "IHDR", "PLTE", "bKGD", "tRNS", "hIST", "cHRM", "gAMA", "sRGB", "iCCP", "sBIT", "pHYs", "sPLT"):
                    raise UnexpectedChunk(kind, "IDAT")
            elif kind == "IHDR":
                raise DuplicateChunk("IHDR")                     # :336-337
            elif kind == "PLTE":                                 # :339-355
                if plte is not None:
                    raise DuplicateChunk("PLTE")
                if bkgd is not None:
                    raise UnexpectedChunk("PLTE", "bKGD")
                if trns is not None:
                    raise UnexpectedChunk("PLTE", "tRNS")
                parsed(kind, value)                              # PNG.Image.swift:355
                plte = payload(e)
                metadata._critical = (plte, bkgd, trns)
                continue
            elif kind in ("bKGD", "tRNS"):                       # PNG.Metadata.swift:173-182
                if (bkgd if kind == "bKGD" else trns) is not None:
                    raise DuplicateChunk(kind)
                parsed(kind, value)
                if kind == "bKGD":
                    bkgd = payload(e)
                else:
                    trns = payload(e)
                metadata._critical = (plte, bkgd, trns)
                continue
            if kind in ("iTXt", "tEXt", "zTXt", "iCCP"):
                if kind == "iCCP" and (plte is not None or metadata.colorProfile is not None):
                    metadata.push((kind, b""), palette_seen=plte is not None)        # (raises: the order and the multiplicity come first)
                if e.status != DONE:
                    raise ParsingError(e.status, (e.aux, 0))
                work.append((e, kind))
                metadata.push((kind, b""), palette_seen=plte is not None, parsed=len(work) - 1)
            else:
                metadata.push((kind, payload(e)), palette_seen=plte is not None, value=value)

    @staticmethod
    def decompress(data, typed=False, session=None) -> Image:
        """PNG.Image.decompress(stream:) (Sources/PNG/PNG.Image.swift:298-400) for a whole file: lexed on the device with its chunk
        directory (spng_lex_dir_batch), the image decoded there from the IDAT bytes the lexer gathered (spng_decode_batch), the heads of
        the text and profile chunks parsed there; their compressed bodies inflated in one spng_inflate_batch call straight from the
        file's bytes in device memory, Latin-1 contents transcoded and iTXt contents checked in one spng_text_batch call.  The host
        sees the infos, the directory, the small chunks and the finished contents; it applies the rules about which chunks may
        stand where (RequiredChunk, DuplicateChunk, UnexpectedChunk) and reads PLTE / tRNS / bKGD.  An iTXt content that is not
        well-formed UTF-8 is repaired on the host with errors="replace".
        typed: every other chunk is parsed on the device as well (spng_parse_dir_batch, enqueued behind the directory with no wait in
        between): the header's ParsingError is raised first (:317), every chunk's behind the rules about its place, PLTE / tRNS /
        bKGD are validated and read from their records, and the metadata's fields are typed (Metadata).  The default answers what
        it always has: a malformed typed chunk travels as it is."""
        from . import (E_OUTPUT_CAPACITY, E_PROFILE_INCOMPLETE, E_TEXT_ENCODING, E_TEXT_INCOMPLETE, FORMAT_IOS, FORMAT_ZLIB,
                       NEED_MORE_INPUT, TEXT_CHECK_UTF8, TEXT_LATIN1_TO_UTF8, ParsingError, load, raise_for, storage_size, inflated_size)
        s = session or load()
        data = bytes(data)
        d_png = s.to_device(data)
        values = None
        if typed:
            (info,), (entries,), (values,), _, _, (d_idat,) = s.lex_parse_batch([data], d_png=[d_png])
        else:
            (info,), (d_idat,), (entries,) = s.lex_dir_batch([data], d_png=[d_png], device_idat=True)
        # (the chunks in front of a lexing failure have been lexed in full: what is wrong with them comes first, as in the reference's loop)
        names = [_name(e.type) for e in entries]
        payload = lambda e: data[e.offset:e.offset + e.length]  # noqa: E731
        # :303-321: CgBI?, IHDR
        at = 1 if names[:1] == ["CgBI"] else 0
        if len(names) <= at:
            raise_for(info.status, (info.aux[0], info.aux[1]))
        if names[at] != "IHDR":
            raise RequiredChunk("IHDR", names[at])
        ios = at == 1
        if typed and values[at].status != DONE:                  # :317: PNG.Header.init(parsing:standard:) throws
            raise ParsingError(values[at].status, tuple(values[at].aux))
        metadata = Metadata()
        work = []                                                # (entry, kind): the text and profile chunks, in file order
        pending = None                                           # the first thing wrong with the chunks: raised once the bodies in front of it have been looked at
        try:
            PNG._walk(entries[at + 1:], names[at + 1:], info, metadata, work, payload, values[at + 1:] if typed else None)
        except (ChunkOrderError, ParsingError) as err:
            pending = err
        plte, bkgd, trns = metadata._critical
        if pending is None:
            raise_for(info.status, (info.aux[0], info.aux[1]))
        # the bodies: compressed ones inflated from the file's bytes in device memory, all at once
        bodies = [d_png[e.offset + e.body_off:e.offset + e.length] for e, _ in work]
        packed = [k for k, (e, _) in enumerate(work) if e.compressed]
        caps = [max(1 << 16, 8 * bodies[k].numel()) for k in packed]
        todo = list(range(len(packed)))
        while todo:
            outs, results = s.inflate_batch([bodies[packed[j]] for j in todo], [caps[j] for j in todo])
            again = []
            for j, out, r in zip(todo, outs, results):
                if r.status == E_OUTPUT_CAPACITY:                # (the reference's output buffer is unbounded)
                    caps[j] *= 4
                    again.append(j)
                    continue
                if r.status == NEED_MORE_INPUT:                  # PNG.Text.swift:161-165, 184-188; PNG.ColorProfile.swift:78-82
                    raise ParsingError(E_PROFILE_INCOMPLETE if work[packed[j]][1] == "iCCP" else E_TEXT_INCOMPLETE)
                raise_for(r.status, (r.aux[0], r.aux[1]))
                bodies[packed[j]] = out[:r.written]
            todo = again
        if pending is not None:
            raise pending
        # the image: the IDAT bytes are where the lexer put them
        if (info.color, info.depth) not in ((0, 1), (0, 2), (0, 4), (0, 8), (0, 16), (2, 8), (2, 16), (3, 1), (3, 2), (3, 4), (3, 8), (4, 8),
                                            (4, 16), (6, 8), (6, 16)) or not info.width or not info.height:
            raise ValueError("no PNG.Header: the pixel format or the size of IHDR")     # (PNG.Header.init(parsing:standard:) throws)
        channels = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}[info.color]
        size = (info.width, info.height)
        d_rows = s.empty(inflated_size(size[0], size[1], info.depth, channels, bool(info.interlace)))
        nbytes = storage_size(size[0], size[1], info.depth, channels)
        d_storage = s.empty(nbytes)
        desc = s.image_desc(d_idat[:info.idat_len], d_rows, d_storage, size[0], size[1], info.depth, channels, bool(info.interlace),
                            FORMAT_IOS if ios else FORMAT_ZLIB)
        (res,) = s.decode_batch([desc])
        raise_for(res.status, (res.aux[0], res.aux[1]))
        if res.status == NEED_MORE_INPUT:
            raise DecodingError(E_INCOMPLETE_DATASTREAM)         # (PNG.Context.swift:137-142)
        storage = bytes(d_storage[:nbytes].cpu().numpy())
        # the contents: Latin-1 ones transcoded, iTXt ones checked
        texts = [k for k, (_, kind) in enumerate(work) if kind != "iCCP"]
        ops = [TEXT_CHECK_UTF8 if work[k][1] == "iTXt" else TEXT_LATIN1_TO_UTF8 for k in texts]
        outs, results = s.text_batch([bodies[k] for k in texts], ops) if texts else ([], [])
        parsed = []
        for k, (e, kind) in enumerate(work):
            raw = payload(e)
            if kind == "iCCP":
                parsed.append(ColorProfile(raw[:e.k].decode("latin-1"), bodies[k].cpu().numpy().tobytes()))
                continue
            out, r = outs[texts.index(k)], results[texts.index(k)]
            english = raw[:e.k].decode("latin-1")
            if kind == "iTXt":
                if r.status not in (DONE, E_TEXT_ENCODING):
                    raise_for(r.status, (r.aux[0], r.aux[1]))
                content = bodies[k].cpu().numpy().tobytes().decode("utf-8", "replace" if r.status == E_TEXT_ENCODING else "strict")
                tag = raw[e.k + 3:e.l]
                language = [t.decode("latin-1").lower() for t in tag.split(b"-")] if tag else []      # PNG.Text.swift:265-286
                localized = raw[e.l + 1:e.m].decode("utf-8", "replace")
                parsed.append(Text(e.compressed, (english, "" if localized == english else localized), language, content))
            else:
                raise_for(r.status, (r.aux[0], r.aux[1]))
                parsed.append(Text(e.compressed, (english, ""), ["en"], out[:r.written].cpu().numpy().tobytes().decode("utf-8")))
        metadata.text = [parsed[k] for k in metadata.text]
        if metadata.colorProfile is not None:
            metadata.colorProfile = parsed[metadata.colorProfile]
        # PNG.Format.recognize (Formats/PNG.Format.swift:396-560): what PLTE / tRNS / bKGD mean for this pixel format
        indexed = info.color == 3
        palette = key = fill = None

        def fields(raw):
            v = struct.unpack(">" + "H" * (len(raw) // 2), raw)
            return v[0] if len(v) == 1 else (v[::-1] if ios else v)

        if typed:                                                # the records: counts and samples as the parsers left them
            rec = metadata._records
            if "PLTE" in rec:
                alphas = trns[:rec["tRNS"].count] if indexed and "tRNS" in rec else b""
                palette = [(plte[3 * k], plte[3 * k + 1], plte[3 * k + 2], alphas[k] if k < len(alphas) else 255) for k in range(rec["PLTE"].count)]
            samples = lambda v: v.v[0] if info.color in (0, 4) else (tuple(v.v[:3])[::-1] if ios else tuple(v.v[:3]))  # noqa: E731
            if "tRNS" in rec and not indexed:
                key = samples(rec["tRNS"])
            if "bKGD" in rec:
                fill = rec["bKGD"].v[0] if indexed else samples(rec["bKGD"])
        elif plte is not None:
            alphas = trns if indexed and trns is not None else b""
            palette = [(plte[3 * k], plte[3 * k + 1], plte[3 * k + 2], alphas[k] if k < len(alphas) else 255) for k in range(len(plte) // 3)]
        if not typed and trns is not None and not indexed:
            key = fields(trns)
        if not typed and bkgd is not None:
            fill = bkgd[0] if indexed else fields(bkgd)
        return Image(size, info.depth, channels, indexed, ios, bool(info.interlace), palette, key, fill, storage, metadata)

    @staticmethod
    def compress(storage, size, depth, channels, indexed=False, bgr=False, interlaced=False, palette=None, key=None, fill=None,
                 before=(), after=(), level=9, chunk_bytes=65544, session=None, metadata=None) -> bytes:
        """PNG.Image.compress(stream:level:hint:) from storage (Sources/PNG/PNG.Image.swift:576-668): -> the bytes of the file, written
        on the device by one spng_compress_batch call.  before / after: the metadata's chunks as (type, payload) pairs, in front of
        PLTE / behind tRNS (the reference's cHRM gAMA sRGB iCCP sBIT, and hIST pHYs tIME iTXt sPLT and application chunks).
        chunk_bytes: payload bytes of every IDAT but the last -- the reference cuts at twice the capacity its output buffer got
        (LZ77.DeflatorOut.swift:15-24, 121), an allocator fact: 65544 at the default hint on Linux, 8200 at hint 4096."""
        from . import load, raise_for
        s = session or load()
        if metadata is not None:
            # metadata: a PNG.Metadata, written in the order of PNG.Image.swift:596-656 in front of `before` / `after`; the profile and
            # the contents of the compressed texts are deflated on the device in one call (LZ77.Deflator(level: 13, exponent: 15),
            # PNG.Text.swift:336, PNG.ColorProfile.swift:97)
            plain = metadata.to_deflate()
            streams = []
            if plain:
                outs, results = s.deflate_batch([s.to_device(p) for p in plain], 13)
                for out, r in zip(outs, results):
                    raise_for(r.status, (r.aux[0], r.aux[1]))
                    streams.append(out[:r.written].cpu().numpy().tobytes())
            m_before, m_after = metadata.chunks(streams)
            before, after = m_before + list(before), m_after + list(after)
        return s.compress(bytes(storage), size, depth, channels, level=level, indexed=indexed, bgr=bgr, interlaced=interlaced, palette=palette,
                          key=key, fill=fill, before=before, after=after, chunk_bytes=chunk_bytes)

    class Context:
        """PNG.Context (Sources/PNG/Decoding/PNG.Context.swift:56-147), image side reduced to the
        fields that cross the boundary: size, pixel depth/channels, interlacing, standard."""

        def __init__(self, size, depth, channels, interlaced=False, standard=FORMAT_ZLIB, session=None):
            from . import load, storage_size, inflated_size
            self._s = session or load()
            self.size, self.depth, self.channels = tuple(size), depth, channels
            self.interlaced, self.standard = bool(interlaced), standard
            self._storage_bytes = storage_size(size[0], size[1], depth, channels)
            self._storage = bytes(self._storage_bytes)
            self._stale = False                  # the device raster is ahead of the host copy
            self._continue = True                # PNG.Decoder.continue (:22-23)
            # device state kept between pushes: the IDAT bytes so far, the inflated scanlines so far (they are the next
            # push's LZ77 window: never defiltered in place), the defiltered scanlines of interlaced / sub-byte images, the
            # raster; and PNG.Decoder.row / pass as the number of inflated bytes already defiltered
            s = self._s
            self._U = inflated_size(size[0], size[1], depth, channels, self.interlaced)
            self._d_idat, self._n_idat = None, 0
            self._d_rows = s.empty(self._U + 64)     # (64 bytes of slack: a little too much data shows as `written > U`)
            direct = not self.interlaced and depth * channels >= 8
            self._d_work = None if direct else s.empty(self._U + 64)
            self._d_storage = s.to_device(self._storage) if self._storage_bytes else s.empty(1)
            self._state = (0, 0, 0, 0)
            self._defiltered = 0
            self.defiltered_total = 0            # scanline bytes handed to the defilter over all pushes (each row once: == U at the end)

        @property
        def storage(self) -> bytes:
            """PNG.Image.storage so far (fetched from the device when it is asked for)"""
            if self._stale:
                self._storage = bytes(self._d_storage[:self._storage_bytes].cpu().numpy())
                self._stale = False
            return self._storage

        def push(self, data: bytes, overdraw: bool = False):
            """push(data:overdraw:) (:88-102): one call per IDAT chunk.  overdraw: the assigned pixels of an unfinished interlaced
            image are replicated over the cells the later passes refine (PNG.Image.overdraw, PNG.Image.swift:134-183), on the
            device (SPNG_IMAGE_OVERDRAW).  The inflate goes on where the previous chunk stopped
            (spng_inflate_resume_batch); the scanlines that became complete with this chunk -- and only those -- are defiltered
            and assigned (spng_unfilter_resume_batch, PNG.Decoder.swift:88-94, 121-135)."""
            if not self._continue:
                raise DecodingError(E_EXTRANEOUS_COMPRESSED_DATA)     # PNG.Decoder.swift:51-55
            s = self._s
            need = self._n_idat + len(data)
            if self._d_idat is None or self._d_idat.numel() < need:
                grown = s.empty(max(2 * need, 1 << 16))
                if self._n_idat:
                    grown[:self._n_idat] = self._d_idat[:self._n_idat]
                self._d_idat = grown
            if data:
                self._d_idat[self._n_idat:need] = s.to_device(bytes(data))
            self.push_device(self._d_idat, need, overdraw)

        def push_device(self, d_idat, length: int, overdraw: bool = False):
            """push(data:overdraw:) for IDAT bytes that are on the device already: d_idat holds ALL IDAT bytes so far, `length` of
            them -- the buffer spng_lex_resume_batch fills, at its idat_len (PNG.decode_online); what lies behind the previous
            push's length is the data of this one."""
            from . import raise_for, E_EXTRANEOUS_IMAGE_DATA
            if not self._continue:
                raise DecodingError(E_EXTRANEOUS_COMPRESSED_DATA)     # PNG.Decoder.swift:51-55
            s = self._s
            self._d_idat, self._n_idat = d_idat, int(length)
            res, state = s.inflate_resume(self._d_idat, self._n_idat, self._d_rows, self.standard, self._state)
            status = res.status
            # PNG.Decoder.swift:142-147: anything left in the inflator after the last row
            if status == E_OUTPUT_CAPACITY or (status in (DONE, NEED_MORE_INPUT) and res.written > self._U):
                status = E_EXTRANEOUS_IMAGE_DATA
            raise_for(status, (res.aux[0], res.aux[1]))
            self._state = state
            w, h = self.size
            now = min(res.written, self._U)
            if now > self._defiltered:
                desc = s.image_desc(None, self._d_rows, self._d_storage, w, h, self.depth, self.channels, self.interlaced,
                                    self.standard, rows_cap=self._d_rows.numel())
                desc.reserved = IMAGE_OVERDRAW if overdraw else 0
                ures = s.unfilter_resume(desc, self._d_work, self._defiltered, now)
                raise_for(ures.status, (ures.aux[0], ures.aux[1]))
                self.defiltered_total += ures.written
                self._defiltered = now
                self._stale = self._stale or ures.written > 0
            self._continue = status == NEED_MORE_INPUT

        def push_ancillary_iend(self):
            """push(ancillary: IEND) (:137-142)."""
            if self._continue:
                raise DecodingError(E_INCOMPLETE_DATASTREAM)

    @staticmethod
    def decode_online(pieces, overdraw=False, capture=None, session=None):
        """decodeOnline of the reference's tutorial (Snippets/PNG/OnlineDecoding.swift:102-216) from the bytes of a file as they arrive:
        every piece of `pieces` is appended to a device buffer and lexed there (spng_lex_resume_batch: waitSignature / waitChunk --
        the truncation statuses are the tutorial's "try again"; every byte is summed and copied once whatever the pieces are); the
        context is made once IHDR and the first IDAT are in; the IDAT bytes whose chunks' checksums have been verified go to
        PNG.Context.push on the device, chunk by chunk; capture(context) is called after every IDAT chunk, as the tutorial writes
        its snapshots, however many of them a piece completes; at IEND, push(ancillary:).  Lexing errors are raised once
        they are final, and for a file that ends early.  -> (context, the last Lexed, PLTE bytes, tRNS bytes); the palette and the
        transparency are read by the host at the offsets reported, as for whole files."""
        from . import (DONE, E_TRUNCATED_CHUNK_BODY, E_TRUNCATED_CHUNK_HEADER, E_TRUNCATED_SIGNATURE, FORMAT_IOS, FORMAT_ZLIB, LexingError,
                       load, raise_for)
        s = session or load()
        waits = (E_TRUNCATED_SIGNATURE, E_TRUNCATED_CHUNK_HEADER, E_TRUNCATED_CHUNK_BODY)
        (state,) = s.lex_states(1)
        d_png, d_idat, n_png, pushed = s.empty(1 << 16), s.empty(1 << 16), 0, 0
        context, info, head = None, None, bytearray()
        for piece in pieces:
            piece = bytes(piece)
            if not piece:
                continue
            need = n_png + len(piece)
            if d_png.numel() < need:
                # (both buffers whole: the payload of the chunk in progress is copied ahead of idat_len)
                grown, grown_idat = s.empty(2 * need), s.empty(2 * need)
                grown[:n_png] = d_png[:n_png]
                grown_idat[:d_idat.numel()] = d_idat
                d_png, d_idat = grown, grown_idat
            d_png[n_png:need] = s.to_device(piece)
            n_png = need
            if context is None:
                head += piece                            # (what the host reads PLTE / tRNS from: they stand in front of the first IDAT)
            # waitChunk: a chunk at a time, as the tutorial lexes -- the lexer is asked for the bytes up to the end of the chunk in
            # progress (its place and length are in the last answer), so that a piece that completes several IDAT chunks still shows
            # the image after each of them.  Every byte is summed and copied once all the same: the state goes on where it stopped.
            while True:
                upto = n_png
                if info is not None and info.status == E_TRUNCATED_CHUNK_BODY:
                    upto = min(n_png, info.consumed + 8 + info.aux[0])
                elif info is not None and info.status == E_TRUNCATED_CHUNK_HEADER:
                    upto = min(n_png, info.consumed + 8)
                (info,) = s.lex_resume_batch([(d_png, upto, d_idat)], [state])
                if info.status != DONE and info.status not in waits:
                    raise_for(info.status, (info.aux[0], info.aux[1]))
                if context is None and (info.idat_len or info.status == DONE):
                    channels = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}[info.color]
                    context = PNG.Context((info.width, info.height), info.depth, channels, bool(info.interlace),
                                          FORMAT_IOS if info.ios else FORMAT_ZLIB, session=s)
                if info.idat_len > pushed:
                    context.push_device(d_idat, info.idat_len, overdraw)
                    pushed = info.idat_len
                    if capture is not None:
                        capture(context)
                if info.status == DONE:
                    context.push_ancillary_iend()
                    plte = bytes(head[info.plte_off:info.plte_off + info.plte_len])
                    trns = bytes(head[info.trns_off:info.trns_off + info.trns_len])
                    return context, info, plte, trns
                if upto == n_png:
                    break
        raise LexingError(info.status if info is not None else E_TRUNCATED_SIGNATURE, (info.aux[0], 0) if info is not None else (0, 0))
