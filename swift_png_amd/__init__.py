"""swift_png_amd -- host-side mirror of swift-png's hot-path API over libspng_mi355.so.

The product is the C-ABI library (include/spng_mi355.h, built from swift_png_amd/csrc/*.hip for
gfx950).  swift-png itself is Swift; no Swift toolchain exists in this environment, so the host
code above the C ABI is Python and mirrors the reference's seams for this path:

    LZ77.Inflator              Sources/LZ77/Inflator/LZ77.Inflator.swift:8-62
    PNG.Decoder.defilter       Sources/PNG/Decoding/PNG.Decoder.swift:152-196
    PNG.Encoder.filter         Sources/PNG/Encoding/PNG.Encoder.swift:132-204
    PNG.Context.push(data:)    Sources/PNG/Decoding/PNG.Context.swift:88-147

PyTorch is used only for device memory and streams.  There is no CPU fallback: `load()` raises
when the HIP library or the GPU is missing.
"""
from __future__ import annotations

import ctypes
import os
from pathlib import Path

_HERE = Path(__file__).resolve().parent
LIB_PATH = Path(os.environ.get("SPNG_LIB", _HERE / "libspng_mi355.so"))   # SPNG_LIB: tuning builds only

# ---- status vocabulary (include/spng_mi355.h) -------------------------------------------------
DONE, NEED_MORE_INPUT = 0, 1
E_COMPRESSION_METHOD, E_WINDOW_SIZE, E_CHECK_BITS, E_DICTIONARY = 16, 17, 18, 19
E_GZIP_SIGIL, E_GZIP_METHOD, E_GZIP_FLAG_BITS, E_GZIP_HEADER_CHECKSUM = 24, 25, 26, 27
(E_STREAM_CHECKSUM, E_BLOCK_TYPE, E_BLOCK_COUNT_PARITY, E_RUNLITERAL_COUNT, E_CODELENGTH_TABLE,
 E_CODELENGTH_SEQUENCE, E_HUFFMAN_TABLE, E_STRING_REFERENCE) = range(32, 40)
E_EXTRANEOUS_IMAGE_DATA, E_EXTRANEOUS_COMPRESSED_DATA, E_INCOMPLETE_DATASTREAM = 48, 49, 50
E_OUTPUT_CAPACITY, E_ARGUMENT, E_DEVICE, E_REFERENCE_UNDEFINED = 64, 65, 66, 67
(E_TRUNCATED_SIGNATURE, E_SIGNATURE, E_TRUNCATED_CHUNK_HEADER, E_TRUNCATED_CHUNK_BODY, E_CHUNK_TYPE,
 E_CHUNK_CHECKSUM) = range(80, 86)
(E_TEXT_KEYWORD, E_TEXT_CHUNK_LENGTH, E_TEXT_LANGUAGE, E_TEXT_LOCALIZED_KEYWORD, E_TEXT_COMPRESSION_METHOD, E_TEXT_COMPRESSION,
 E_TEXT_INCOMPLETE) = range(96, 103)
E_PROFILE_NAME, E_PROFILE_CHUNK_LENGTH, E_PROFILE_COMPRESSION_METHOD, E_PROFILE_INCOMPLETE = range(104, 108)
E_TEXT_ENCODING = 112
# the other 33 cases of PNG.ParsingError, in the order of its enum: the status of a ChunkValue (spng_parse_dir_batch)
(E_PARSE_HEADER_CHUNK_LENGTH, E_PARSE_HEADER_PIXEL_FORMAT_CODE, E_PARSE_HEADER_PIXEL_FORMAT, E_PARSE_HEADER_COMPRESSION_METHOD,
 E_PARSE_HEADER_FILTER, E_PARSE_HEADER_INTERLACING, E_PARSE_HEADER_SIZE, E_PARSE_UNEXPECTED_PALETTE, E_PARSE_PALETTE_CHUNK_LENGTH,
 E_PARSE_PALETTE_COUNT, E_PARSE_UNEXPECTED_TRANSPARENCY, E_PARSE_TRANSPARENCY_CHUNK_LENGTH, E_PARSE_TRANSPARENCY_SAMPLE,
 E_PARSE_TRANSPARENCY_COUNT, E_PARSE_BACKGROUND_CHUNK_LENGTH, E_PARSE_BACKGROUND_SAMPLE, E_PARSE_BACKGROUND_INDEX,
 E_PARSE_HISTOGRAM_CHUNK_LENGTH, E_PARSE_GAMMA_CHUNK_LENGTH, E_PARSE_CHROMATICITY_CHUNK_LENGTH, E_PARSE_RENDERING_CHUNK_LENGTH,
 E_PARSE_RENDERING_CODE, E_PARSE_SIGNIFICANT_BITS_CHUNK_LENGTH, E_PARSE_SIGNIFICANT_BITS_PRECISION, E_PARSE_PHYSICAL_CHUNK_LENGTH,
 E_PARSE_PHYSICAL_UNIT, E_PARSE_SUGGESTED_PALETTE_CHUNK_LENGTH, E_PARSE_SUGGESTED_PALETTE_NAME, E_PARSE_SUGGESTED_PALETTE_DATA_LENGTH,
 E_PARSE_SUGGESTED_PALETTE_DEPTH, E_PARSE_SUGGESTED_PALETTE_FREQUENCY, E_PARSE_TIME_CHUNK_LENGTH, E_PARSE_TIME) = range(128, 161)
SCOPE_NONE, SCOPE_PARSED, SCOPE_NO_HEADER, SCOPE_NO_PALETTE = 0, 1, 2, 3
NO_OFFSET = 0xffffffff
TEXT_LATIN1_TO_UTF8, TEXT_CHECK_UTF8 = 1, 2
TEXT_TILE = 4096                                            # csrc/text.hip: bytes of a tile (the tests place their boundaries by it)
FORMAT_ZLIB, FORMAT_IOS, FORMAT_GZIP = 0, 1, 2
K_INFLATE, K_UNFILTER, K_SCATTER, K_FILTER, K_DEFLATE, K_ADLER, K_PINFLATE = 0, 1, 2, 3, 4, 5, 6
K_UNPACK = 7
K_PACK = 10
IMAGE_OVERDRAW = 1
TARGET_RGBA, TARGET_VA, TARGET_SCALAR = 0, 1, 2
PREMULTIPLY, PREMULTIPLY_AS_U8, STRAIGHTEN, STRAIGHTEN_AS_U8 = 1, 2, 3, 4
K_LEX = 12
K_PINF_FIND, K_PINF_DECODE, K_PINF_RESOLVE = 8, 9, 11
K_DFL_SEARCH, K_DFL_PARSE = 13, 14
K_ALPHA = 15
K_CENSUS, K_PACK_INDEXED = 16, 17
K_HSVA = 18
HSVA_FROM_RGBA8, HSVA_TO_RGBA8, HSVA_TO_VA8 = 1, 2, 3
_HSVA_BYTES = {1: (4, 8), 2: (8, 4), 3: (8, 2)}             # op: bytes of a pixel in, out
K_LUMINANCE = 19
LUMINANCE_V8, LUMINANCE_VA8 = 1, 2                          # (the op is also the bytes of a pixel coming out; 4 go in)
# thresholds of csrc/indexing.hip (the tests take the sizes at which the kernels change paths from here)
CENSUS_LDS_SLOTS, CENSUS_LDS_LIMIT = 2048, 512     # a workgroup's table; keys in it above which it is merged into the image's
CENSUS_FINISH_LDS_KEYS = 4096                      # up to so many keys are sorted in LDS, more in the context's scratch
PACK_INDEXED_LDS_KEYS = 512                        # maps of up to so many keys sit in an LDS hash table, larger ones are searched
# thresholds of csrc/colour_tables.hip (tests/test_colour_tables_host.py compares them with the source's)
CENSUS_WIDE_CAP = 1 << 24                          # keys of a wide census, and of a map
CENSUS_WIDE_TILE = 4096                            # elements a workgroup sorts in LDS; every stride from here on is a launch of its own
MAP_LDS_KEYS, MAP_LDS_SLOTS = 512, 2048            # maps of up to so many keys sit in an LDS hash table (of so many slots),
MAP_MIN_SLOTS = 64                                 # larger ones in scratch: max(this, 2 x map_count rounded up to a power of two) slots
CFG_INFLATE_MODE, CFG_SEGMENT_BYTES, CFG_TOKEN_BYTES, CFG_UNFILTER_PIECE_ROWS, CFG_RESOLVE_PARTS = 0, 1, 2, 3, 5          # (4: reserved)
CFG_DEFLATE_BYTES, CFG_MULTI_GROUPS = 7, 8          # (6: reserved)
CFG_BLOCK_CUT_BYTES = 9                            # parallel inflate: shortest run of segments without a block start that is cut (bytes; 0: 1 MiB)
BLOCK_CUT_AUTO, BLOCK_CUT_NEVER = 0, 1
INFLATE_AUTO, INFLATE_SERIAL = 0, 1

EXPORTS = [
    "spng_version", "spng_status_string", "spng_last_error_string", "spng_inflated_size",
    "spng_storage_size", "spng_create", "spng_destroy", "spng_stream", "spng_sync", "spng_profile",
    "spng_profile_get", "spng_token_stats", "spng_cut_stats", "spng_configure", "spng_inflate_batch", "spng_inflate_resume_batch", "spng_unfilter_batch",
    "spng_unfilter_resume_batch", "spng_decode_batch",
    "spng_inflate", "spng_unfilter", "spng_decode", "spng_adler32", "spng_filter_batch", "spng_filter",
    "spng_lex_batch", "spng_write_idat_batch", "spng_crc32", "spng_unpack_batch", "spng_unpack", "spng_unpack_as", "spng_pack_batch", "spng_pack_as", "spng_alpha_batch", "spng_alpha", "spng_hsva_batch", "spng_hsva", "spng_luminance_batch", "spng_luminance", "spng_census_batch", "spng_census", "spng_pack_indexed_batch", "spng_pack_indexed", "spng_census_wide_batch", "spng_census_wide", "spng_map_batch", "spng_map", "spng_deflate_bound", "spng_deflate_batch", "spng_deflate", "spng_deflate_window", "spng_encode_batch",
    "spng_shard", "spng_decode_batch_multi", "spng_copy_ceiling", "spng_trim", "spng_lds_exchange_ordered", "spng_deflate_state_bytes", "spng_deflate_resume_batch",
    "spng_lex_state_bytes", "spng_lex_resume_batch", "spng_lex_resume_stats",
    "spng_file_bound", "spng_write_file_batch", "spng_compress_batch",
    "spng_lex_dir_batch", "spng_text_batch", "spng_parse_dir_batch",
]


def source_digest() -> str:
    """sha256 (first 16 hex digits) over the kernel sources and the ABI header: what a measurement file (profiles/*_pmc_*.json)
    names as the build it was taken on, and what bench.py compares with the sources it runs"""
    import hashlib
    h = hashlib.sha256()
    root = Path(__file__).resolve().parent
    for f in sorted(list((root / "csrc").glob("*.hip")) + list((root / "csrc").glob("*.hpp")) + list((root.parent / "include").glob("*.h"))):
        h.update(f.name.encode()); h.update(f.read_bytes())
    return h.hexdigest()[:16]


class Result(ctypes.Structure):
    _fields_ = [("status", ctypes.c_int32), ("reserved", ctypes.c_int32), ("written", ctypes.c_uint64),
                ("consumed", ctypes.c_uint64), ("aux", ctypes.c_uint64 * 2)]


class StreamDesc(ctypes.Structure):
    _fields_ = [("d_src", ctypes.c_void_p), ("src_len", ctypes.c_uint64), ("d_dst", ctypes.c_void_p),
                ("dst_cap", ctypes.c_uint64), ("format", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class ImageDesc(ctypes.Structure):
    _fields_ = [("d_idat", ctypes.c_void_p), ("idat_len", ctypes.c_uint64), ("d_rows", ctypes.c_void_p),
                ("rows_cap", ctypes.c_uint64), ("d_storage", ctypes.c_void_p), ("width", ctypes.c_uint32),
                ("height", ctypes.c_uint32), ("depth", ctypes.c_uint8), ("channels", ctypes.c_uint8),
                ("interlaced", ctypes.c_uint8), ("format", ctypes.c_uint8), ("reserved", ctypes.c_uint32)]


class FileDesc(ctypes.Structure):
    _fields_ = [("d_png", ctypes.c_void_p), ("len", ctypes.c_uint64), ("d_idat", ctypes.c_void_p), ("idat_cap", ctypes.c_uint64)]


class Lexed(ctypes.Structure):
    _fields_ = [("status", ctypes.c_int32), ("chunks", ctypes.c_uint32), ("aux", ctypes.c_uint64 * 2),
                ("width", ctypes.c_uint32), ("height", ctypes.c_uint32), ("depth", ctypes.c_uint8), ("color", ctypes.c_uint8),
                ("compression", ctypes.c_uint8), ("filter", ctypes.c_uint8), ("interlace", ctypes.c_uint8),
                ("ios", ctypes.c_uint8), ("pad", ctypes.c_uint8 * 2), ("idat_len", ctypes.c_uint64),
                ("plte_off", ctypes.c_uint64), ("trns_off", ctypes.c_uint64), ("plte_len", ctypes.c_uint32),
                ("trns_len", ctypes.c_uint32), ("consumed", ctypes.c_uint64)]


class ChunkEntry(ctypes.Structure):
    _fields_ = [("type", ctypes.c_uint32), ("length", ctypes.c_uint32), ("offset", ctypes.c_uint64), ("status", ctypes.c_int32),
                ("aux", ctypes.c_uint32), ("k", ctypes.c_uint32), ("l", ctypes.c_uint32), ("m", ctypes.c_uint32),
                ("body_off", ctypes.c_uint32), ("compressed", ctypes.c_uint8), ("pad", ctypes.c_uint8 * 7)]


class ChunkDir(ctypes.Structure):
    _fields_ = [("d_entries", ctypes.c_void_p), ("cap", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


class ChunkValue(ctypes.Structure):
    _fields_ = [("status", ctypes.c_int32), ("scope", ctypes.c_uint32), ("aux", ctypes.c_uint64 * 2), ("count", ctypes.c_uint32),
                ("k", ctypes.c_uint32), ("v", ctypes.c_uint32 * 8)]


class Parsed(ctypes.Structure):
    _fields_ = [("status", ctypes.c_int32), ("index", ctypes.c_uint32), ("aux", ctypes.c_uint64 * 2), ("ihdr_index", ctypes.c_uint32),
                ("plte_index", ctypes.c_uint32), ("palette_count", ctypes.c_uint32), ("depth", ctypes.c_uint8), ("color", ctypes.c_uint8),
                ("ios", ctypes.c_uint8), ("interlaced", ctypes.c_uint8)]


class TextDesc(ctypes.Structure):
    _fields_ = [("d_in", ctypes.c_void_p), ("len", ctypes.c_uint64), ("d_out", ctypes.c_void_p), ("out_cap", ctypes.c_uint64),
                ("op", ctypes.c_uint8), ("reserved", ctypes.c_uint8 * 7)]


class UnpackDesc(ctypes.Structure):
    _fields_ = [("d_storage", ctypes.c_void_p), ("d_out", ctypes.c_void_p), ("d_palette", ctypes.c_void_p),
                ("width", ctypes.c_uint32), ("height", ctypes.c_uint32), ("palette_count", ctypes.c_uint32),
                ("key", ctypes.c_uint16 * 3), ("depth", ctypes.c_uint8), ("channels", ctypes.c_uint8), ("indexed", ctypes.c_uint8),
                ("bgr", ctypes.c_uint8), ("has_key", ctypes.c_uint8), ("target", ctypes.c_uint8), ("layout", ctypes.c_uint8),
                ("premultiply", ctypes.c_uint8), ("reserved", ctypes.c_uint8 * 6)]


class PackDesc(ctypes.Structure):
    _fields_ = [("d_pixels", ctypes.c_void_p), ("d_storage", ctypes.c_void_p), ("d_palette", ctypes.c_void_p),
                ("width", ctypes.c_uint32), ("height", ctypes.c_uint32), ("palette_count", ctypes.c_uint32),
                ("depth", ctypes.c_uint8), ("channels", ctypes.c_uint8), ("indexed", ctypes.c_uint8), ("bgr", ctypes.c_uint8),
                ("source", ctypes.c_uint8), ("layout", ctypes.c_uint8), ("premultiply", ctypes.c_uint8),
                ("reserved", ctypes.c_uint8 * 5)]


class AlphaDesc(ctypes.Structure):
    _fields_ = [("d_in", ctypes.c_void_p), ("d_out", ctypes.c_void_p), ("count", ctypes.c_uint64), ("bits", ctypes.c_uint8),
                ("layout", ctypes.c_uint8), ("op", ctypes.c_uint8), ("reserved", ctypes.c_uint8 * 5)]


class HsvaDesc(ctypes.Structure):
    _fields_ = [("d_in", ctypes.c_void_p), ("d_out", ctypes.c_void_p), ("count", ctypes.c_uint64), ("op", ctypes.c_uint8),
                ("reserved", ctypes.c_uint8 * 7)]


class LuminanceDesc(ctypes.Structure):
    _fields_ = [("d_in", ctypes.c_void_p), ("d_out", ctypes.c_void_p), ("count", ctypes.c_uint64), ("op", ctypes.c_uint8),
                ("reserved", ctypes.c_uint8 * 7)]


class CensusDesc(ctypes.Structure):
    _fields_ = [("d_pixels", ctypes.c_void_p), ("count", ctypes.c_uint64), ("d_keys", ctypes.c_void_p), ("d_counts", ctypes.c_void_p),
                ("cap", ctypes.c_uint32), ("bits", ctypes.c_uint8), ("layout", ctypes.c_uint8), ("premultiply", ctypes.c_uint8),
                ("reserved", ctypes.c_uint8 * 1)]


class PackIndexedDesc(ctypes.Structure):
    _fields_ = [("d_pixels", ctypes.c_void_p), ("d_storage", ctypes.c_void_p), ("d_keys", ctypes.c_void_p),
                ("d_indices", ctypes.c_void_p), ("width", ctypes.c_uint32), ("height", ctypes.c_uint32),
                ("map_count", ctypes.c_uint32), ("source", ctypes.c_uint8), ("layout", ctypes.c_uint8),
                ("premultiply", ctypes.c_uint8), ("miss", ctypes.c_uint8), ("reserved", ctypes.c_uint8 * 8)]


class MapDesc(ctypes.Structure):
    _fields_ = [("d_pixels", ctypes.c_void_p), ("d_out", ctypes.c_void_p), ("d_keys", ctypes.c_void_p), ("d_values", ctypes.c_void_p),
                ("count", ctypes.c_uint64), ("map_count", ctypes.c_uint32), ("source", ctypes.c_uint8), ("layout", ctypes.c_uint8),
                ("premultiply", ctypes.c_uint8), ("value_bytes", ctypes.c_uint8), ("miss", ctypes.c_uint8 * 8),
                ("reserved", ctypes.c_uint8 * 8)]


class ChunkingDesc(ctypes.Structure):
    _fields_ = [("d_stream", ctypes.c_void_p), ("len", ctypes.c_uint64), ("d_out", ctypes.c_void_p),
                ("out_cap", ctypes.c_uint64), ("chunk_bytes", ctypes.c_uint64)]


class Blob(ctypes.Structure):
    _fields_ = [("type", ctypes.c_uint32), ("len", ctypes.c_uint32), ("data", ctypes.c_void_p)]


class PngDesc(ctypes.Structure):
    _fields_ = [("d_stream", ctypes.c_void_p), ("stream_len", ctypes.c_uint64), ("d_stream_result", ctypes.c_void_p),
                ("stream_cap", ctypes.c_uint64), ("d_out", ctypes.c_void_p), ("out_cap", ctypes.c_uint64), ("chunk_bytes", ctypes.c_uint64),
                ("width", ctypes.c_uint32), ("height", ctypes.c_uint32), ("depth", ctypes.c_uint8), ("channels", ctypes.c_uint8),
                ("indexed", ctypes.c_uint8), ("bgr", ctypes.c_uint8), ("interlaced", ctypes.c_uint8), ("has_key", ctypes.c_uint8),
                ("has_fill", ctypes.c_uint8), ("reserved", ctypes.c_uint8), ("key", ctypes.c_uint16 * 3), ("fill", ctypes.c_uint16 * 3),
                ("palette_count", ctypes.c_uint32), ("palette", ctypes.c_void_p), ("before", ctypes.POINTER(Blob)),
                ("before_count", ctypes.c_uint32), ("after", ctypes.POINTER(Blob)), ("after_count", ctypes.c_uint32)]


def png_desc(size, depth, channels, indexed=False, bgr=False, interlaced=False, palette=None, key=None, fill=None, before=(), after=(),
             chunk_bytes=65544):
    """A spng_png_desc without its device fields, and what keeps its host arrays alive: -> (PngDesc, keep).  palette: bytes or rows of
    (r, g, b, a); key / fill: as PNG.Format holds them -- an int for the grey formats (an indexed format's fill: a palette index),
    (r, g, b), and (b, g, r) for bgr8 / bgra8; before / after: (type, payload) pairs with four-byte types."""
    d, keep = PngDesc(), []
    d.chunk_bytes = int(chunk_bytes)
    d.width, d.height, d.depth, d.channels = int(size[0]), int(size[1]), int(depth), int(channels)
    d.indexed, d.bgr, d.interlaced = int(bool(indexed)), int(bool(bgr)), int(bool(interlaced))
    for name, v in (("key", key), ("fill", fill)):
        if v is not None:
            v = [int(v)] if isinstance(v, int) else [int(x) for x in v]
            setattr(d, "has_" + name, 1)
            setattr(d, name, (ctypes.c_uint16 * 3)(*(v + [0, 0])[:3]))
    if palette is not None and len(palette):
        raw = bytes(palette) if isinstance(palette, (bytes, bytearray, memoryview)) else bytes(x for p in palette for x in p)
        buf = _cbuf(raw)
        keep.append(buf)
        d.palette_count, d.palette = len(raw) // 4, ctypes.addressof(buf)
    for name, blobs in (("before", before), ("after", after)):
        blobs = list(blobs)
        if not blobs:
            continue
        arr = (Blob * len(blobs))()
        for k, (kind, payload) in enumerate(blobs):
            kind, buf = bytes(kind), _cbuf(payload)
            if len(kind) != 4:
                raise SpngError(E_ARGUMENT)
            keep.append(buf)
            arr[k] = Blob(int.from_bytes(kind, "big"), len(bytes(payload)), ctypes.addressof(buf))
        keep.append(arr)
        setattr(d, name, arr)
        setattr(d, name + "_count", len(blobs))
    return d, keep


# ---- error mirror --------------------------------------------------------------------------------
class SpngError(Exception):
    """Base of the mirrored reference errors; `.status` is the C-ABI code, `.aux` its payload."""

    def __init__(self, status, aux=(0, 0)):
        self.status, self.aux = status, tuple(aux)
        super().__init__(f"{_NAMES.get(status, status)}{self.aux if any(self.aux) else ''}")


class StreamHeaderError(SpngError):      # LZ77.StreamHeaderError
    pass


class GzipStreamHeaderError(SpngError):  # Gzip.StreamHeaderError
    pass


class DecompressionError(SpngError):     # LZ77.DecompressionError
    pass


class DecodingError(SpngError):          # PNG.DecodingError
    pass


class LexingError(SpngError):            # PNG.LexingError
    pass


class ParsingError(SpngError):           # PNG.ParsingError
    pass


_NAMES = {
    16: "invalidCompressionMethod", 17: "invalidWindowSize", 18: "invalidCheckBits", 19: "unexpectedDictionary",
    24: "invalidSigil", 25: "invalidCompressionMethod", 26: "invalidFlagBits", 27: "_headerChecksumUnsupported",
    32: "invalidStreamChecksum", 33: "invalidBlockTypeCode", 34: "invalidBlockElementCountParity",
    35: "invalidHuffmanRunLiteralSymbolCount", 36: "invalidHuffmanCodelengthHuffmanTable",
    37: "invalidHuffmanCodelengthSequence", 38: "invalidHuffmanTable", 39: "invalidStringReference",
    48: "extraneousImageData", 49: "extraneousImageDataCompressedData",
    50: "incompleteImageDataCompressedDatastream", 64: "outputCapacity", 65: "invalidArgument",
    66: "deviceError", 67: "referenceUndefined",
    80: "truncatedSignature", 81: "invalidSignature", 82: "truncatedChunkHeader", 83: "truncatedChunkBody",
    84: "invalidChunkTypeCode", 85: "invalidChunkChecksum",
    96: "invalidTextEnglishKeyword", 97: "invalidTextChunkLength", 98: "invalidTextLanguageTag", 99: "invalidTextLocalizedKeyword",
    100: "invalidTextCompressionMethodCode", 101: "invalidTextCompressionCode", 102: "incompleteTextCompressedDatastream",
    104: "invalidColorProfileName", 105: "invalidColorProfileChunkLength", 106: "invalidColorProfileCompressionMethodCode",
    107: "incompleteColorProfileCompressedDatastream", 112: "textEncoding",
    128: "invalidHeaderChunkLength", 129: "invalidHeaderPixelFormatCode", 130: "invalidHeaderPixelFormat",
    131: "invalidHeaderCompressionMethodCode", 132: "invalidHeaderFilterCode", 133: "invalidHeaderInterlacingCode", 134: "invalidHeaderSize",
    135: "unexpectedPalette", 136: "invalidPaletteChunkLength", 137: "invalidPaletteCount", 138: "unexpectedTransparency",
    139: "invalidTransparencyChunkLength", 140: "invalidTransparencySample", 141: "invalidTransparencyCount",
    142: "invalidBackgroundChunkLength", 143: "invalidBackgroundSample", 144: "invalidBackgroundIndex", 145: "invalidHistogramChunkLength",
    146: "invalidGammaChunkLength", 147: "invalidChromaticityChunkLength", 148: "invalidColorRenderingChunkLength",
    149: "invalidColorRenderingCode", 150: "invalidSignificantBitsChunkLength", 151: "invalidSignificantBitsPrecision",
    152: "invalidPhysicalDimensionsChunkLength", 153: "invalidPhysicalDimensionsDensityUnitCode", 154: "invalidSuggestedPaletteChunkLength",
    155: "invalidSuggestedPaletteName", 156: "invalidSuggestedPaletteDataLength", 157: "invalidSuggestedPaletteDepthCode",
    158: "invalidSuggestedPaletteFrequency", 159: "invalidTimeModifiedChunkLength", 160: "invalidTimeModifiedTime",
}


def raise_for(status, aux=(0, 0)):
    if status in (DONE, NEED_MORE_INPUT):
        return
    if 24 <= status < 28:
        raise GzipStreamHeaderError(status, aux)
    if 16 <= status < 32:
        raise StreamHeaderError(status, aux)
    if 32 <= status < 48:
        raise DecompressionError(status, aux)
    if 48 <= status < 64:
        raise DecodingError(status, aux)
    if 80 <= status < 96:
        raise LexingError(status, aux)
    if 96 <= status < 112 or 128 <= status <= 160:
        raise ParsingError(status, aux)
    raise SpngError(status, aux)


# ---- library loading -----------------------------------------------------------------------------
_lib = None


def load_library():
    """dlopens libspng_mi355.so and declares prototypes.  Needs no GPU (used by the symbol tests)."""
    global _lib
    if _lib is not None:
        return _lib
    if not LIB_PATH.exists():
        raise RuntimeError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                           "(hipcc --offload-arch=gfx950); there is no CPU fallback")
    # One HIP runtime per process.  libspng_mi355.so NEEDs libamdhip64.so.7; the torch wheel bundles its
    # own copy with the same SONAME (plus its own HSA runtime).  If the system copy is mapped first and
    # torch is imported afterwards, torch is bound to the system libamdhip64 but still loads its bundled
    # HSA runtime, and device discovery fails ("no ROCm-capable device").  This Python host uses torch for
    # device memory, so torch's runtime goes in first and the library rides it.  A torch-free host (the
    # Swift binding of INTEGRATION.md, tests/test_torch_free.py) simply gets the system runtime.
    import torch  # noqa: F401
    lib = ctypes.CDLL(str(LIB_PATH))
    vp, u64, u32, i32 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int32
    rp = ctypes.POINTER(Result)
    lib.spng_version.restype = i32
    lib.spng_status_string.restype = ctypes.c_char_p
    lib.spng_status_string.argtypes = [i32]
    lib.spng_last_error_string.restype = ctypes.c_char_p
    lib.spng_inflated_size.restype = u64
    lib.spng_inflated_size.argtypes = [u32, u32, ctypes.c_int, ctypes.c_int, ctypes.c_int]
    lib.spng_storage_size.restype = u64
    lib.spng_storage_size.argtypes = [u32, u32, ctypes.c_int, ctypes.c_int]
    lib.spng_create.argtypes = [ctypes.c_int, vp, ctypes.POINTER(vp)]
    lib.spng_destroy.restype = None
    lib.spng_destroy.argtypes = [vp]
    lib.spng_stream.restype = vp
    lib.spng_stream.argtypes = [vp]
    lib.spng_sync.argtypes = [vp]
    lib.spng_configure.argtypes = [vp, ctypes.c_int, ctypes.c_int64]
    lib.spng_profile.argtypes = [vp, ctypes.c_int]
    lib.spng_profile_get.argtypes = [vp, ctypes.c_int, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(u64)]
    lib.spng_token_stats.argtypes = [vp, ctypes.POINTER(u64), ctypes.POINTER(u64), ctypes.POINTER(ctypes.c_int32)]
    lib.spng_cut_stats.argtypes = [vp, ctypes.POINTER(u64), ctypes.POINTER(u64), ctypes.POINTER(u64)]
    lib.spng_inflate_batch.argtypes = [vp, ctypes.POINTER(StreamDesc), u32, vp, rp]
    lib.spng_inflate_resume_batch.argtypes = [vp, ctypes.POINTER(StreamDesc), ctypes.POINTER(ctypes.c_uint64), u32, vp, rp]
    lib.spng_unfilter_batch.argtypes = [vp, ctypes.POINTER(ImageDesc), u32, vp, vp, rp]
    lib.spng_unfilter_resume_batch.argtypes = [vp, ctypes.POINTER(ImageDesc), ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(u64),
                                               ctypes.POINTER(u64), u32, vp, rp]
    lib.spng_decode_batch.argtypes = [vp, ctypes.POINTER(ImageDesc), u32, vp, rp]
    lib.spng_filter_batch.argtypes = [vp, ctypes.POINTER(ImageDesc), u32, vp, rp]
    lib.spng_inflate.argtypes = [vp, vp, u64, i32, vp, u64, rp]
    lib.spng_unfilter.argtypes = [vp, vp, u64, u32, u32, ctypes.c_int, ctypes.c_int, ctypes.c_int, vp, rp]
    lib.spng_decode.argtypes = [vp, vp, u64, i32, u32, u32, ctypes.c_int, ctypes.c_int, ctypes.c_int, vp, rp]
    lib.spng_adler32.argtypes = [vp, vp, u64, ctypes.POINTER(u32)]
    lib.spng_filter.argtypes = [vp, vp, u32, u32, ctypes.c_int, ctypes.c_int, ctypes.c_int, vp, rp]
    lib.spng_lex_batch.argtypes = [vp, ctypes.POINTER(FileDesc), u32, vp, ctypes.POINTER(Lexed)]
    lib.spng_lex_state_bytes.restype = u64
    lib.spng_lex_resume_batch.argtypes = [vp, ctypes.POINTER(FileDesc), ctypes.POINTER(vp), u32, vp, ctypes.POINTER(Lexed)]
    lib.spng_lex_dir_batch.argtypes = [vp, ctypes.POINTER(FileDesc), ctypes.POINTER(ChunkDir), u32, vp, ctypes.POINTER(Lexed)]
    lib.spng_text_batch.argtypes = [vp, ctypes.POINTER(TextDesc), u32, vp, rp]
    lib.spng_parse_dir_batch.argtypes = [vp, ctypes.POINTER(FileDesc), ctypes.POINTER(ChunkDir), vp, ctypes.POINTER(vp), u32, vp,
                                         ctypes.POINTER(Parsed)]
    lib.spng_lex_resume_stats.argtypes = [vp, ctypes.POINTER(u64), ctypes.POINTER(u64), ctypes.POINTER(u64)]
    lib.spng_write_idat_batch.argtypes = [vp, ctypes.POINTER(ChunkingDesc), u32, vp, rp]
    lib.spng_crc32.argtypes = [vp, vp, u64, ctypes.POINTER(u32)]
    lib.spng_file_bound.restype = u64
    lib.spng_file_bound.argtypes = [ctypes.POINTER(PngDesc), u64]
    lib.spng_write_file_batch.argtypes = [vp, ctypes.POINTER(PngDesc), u32, vp, rp]
    lib.spng_compress_batch.argtypes = [vp, ctypes.POINTER(ImageDesc), ctypes.POINTER(PngDesc), i32, u32, vp, rp]
    lib.spng_unpack_batch.argtypes = [vp, vp, u32]
    lib.spng_unpack.argtypes = [vp, vp, u32, u32, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                vp, u32, vp, vp]
    lib.spng_unpack_as.argtypes = [vp, vp, u32, u32, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                   ctypes.c_int, ctypes.c_int, vp, u32, vp, vp]
    lib.spng_pack_batch.argtypes = [vp, vp, u32]
    lib.spng_pack_as.argtypes = [vp, vp, u32, u32, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                 ctypes.c_int, vp, u32, vp]
    lib.spng_alpha_batch.argtypes = [vp, vp, u32, vp, rp]
    lib.spng_alpha.argtypes = [vp, vp, u64, ctypes.c_int, ctypes.c_int, ctypes.c_int, vp, rp]
    lib.spng_hsva_batch.argtypes = [vp, vp, u32, vp, rp]
    lib.spng_hsva.argtypes = [vp, vp, u64, ctypes.c_int, vp, rp]
    lib.spng_luminance_batch.argtypes = [vp, vp, u32, vp, rp]
    lib.spng_luminance.argtypes = [vp, vp, u64, ctypes.c_int, vp, rp]
    lib.spng_census_batch.argtypes = [vp, vp, u32, vp, rp]
    lib.spng_census.argtypes = [vp, vp, u64, ctypes.c_int, ctypes.c_int, ctypes.c_int, u32, vp, vp, rp]
    lib.spng_pack_indexed_batch.argtypes = [vp, vp, u32, vp, rp]
    lib.spng_pack_indexed.argtypes = [vp, vp, u32, u32, ctypes.c_int, ctypes.c_int, ctypes.c_int, vp, vp, u32, ctypes.c_int, vp, rp]
    lib.spng_census_wide_batch.argtypes = [vp, vp, u32, vp, rp]
    lib.spng_census_wide.argtypes = [vp, vp, u64, ctypes.c_int, ctypes.c_int, ctypes.c_int, u32, vp, vp, rp]
    lib.spng_map_batch.argtypes = [vp, vp, u32, vp, rp]
    lib.spng_map.argtypes = [vp, vp, u64, ctypes.c_int, ctypes.c_int, ctypes.c_int, vp, vp, u32, ctypes.c_int, vp, vp, rp]
    lib.spng_deflate_bound.restype = u64
    lib.spng_deflate_bound.argtypes = [u64]
    lib.spng_deflate_batch.argtypes = [vp, ctypes.POINTER(StreamDesc), ctypes.POINTER(i32), u32, vp, rp]
    lib.spng_deflate.argtypes = [vp, vp, u64, i32, i32, vp, u64, rp]
    lib.spng_deflate_window.argtypes = [vp, vp, u64, i32, i32, i32, vp, u64, rp]
    lib.spng_encode_batch.argtypes = [vp, ctypes.POINTER(ImageDesc), i32, u32, vp, rp]
    lib.spng_deflate_state_bytes.restype = u64
    lib.spng_deflate_resume_batch.argtypes = [vp, ctypes.POINTER(StreamDesc), ctypes.POINTER(i32), ctypes.POINTER(vp), ctypes.POINTER(ctypes.c_uint8),
                                              ctypes.POINTER(u64), u32, vp, rp]
    lib.spng_shard.argtypes = [u32, u32, u32, ctypes.POINTER(u32), ctypes.POINTER(u32)]
    lib.spng_decode_batch_multi.argtypes = [ctypes.POINTER(vp), u32, ctypes.POINTER(ImageDesc), u32, ctypes.POINTER(vp), rp]
    lib.spng_copy_ceiling.argtypes = [vp, vp, vp, u64, i32, i32, ctypes.POINTER(ctypes.c_double)]
    lib.spng_trim.argtypes = [vp]
    for name in EXPORTS:
        getattr(lib, name)
    _lib = lib
    return lib


_sessions = {}


def load(device: int = 0) -> "Session":
    """Returns the process-wide Session for `device`; raises if the HIP path cannot run."""
    if device not in _sessions:
        _sessions[device] = Session(device)
    return _sessions[device]


def shard_of(count: int, parts: int, index: int):
    """(first, n) of block `index` when `count` images are cut into `parts` contiguous blocks (spng_shard)"""
    first, n = ctypes.c_uint32(0), ctypes.c_uint32(0)
    lib = load_library()
    _check(lib, lib.spng_shard(count, parts, index, ctypes.byref(first), ctypes.byref(n)))
    return first.value, n.value


def decode_batch_multi(sessions, descs, gather=None):
    """spng_decode_batch_multi: `descs` (ImageDesc, device pointers on the device of each block's session) decoded by the
    sessions' contexts, block k by sessions[k]; gather: per image a device pointer on sessions[0]'s device (or 0 / None)
    where its raster is wanted.  -> list[Result]"""
    lib = load_library()
    n = len(descs)
    arr = descs if isinstance(descs, ctypes.Array) else (ImageDesc * n)(*descs)
    ctxs = (ctypes.c_void_p * len(sessions))(*[s.ctx for s in sessions])
    res = (Result * n)()
    g = None
    if gather is not None:
        g = (ctypes.c_void_p * n)(*[int(x) if x else None for x in gather])
    _check(lib, lib.spng_decode_batch_multi(ctxs, len(sessions), arr, n, g, res))
    return list(res)


def inflated_size(w, h, depth, channels, interlaced) -> int:
    return load_library().spng_inflated_size(w, h, depth, channels, int(bool(interlaced)))


def storage_size(w, h, depth, channels) -> int:
    return load_library().spng_storage_size(w, h, depth, channels)


def _check(lib, st):
    if st != DONE:
        msg = lib.spng_last_error_string().decode() if st == E_DEVICE else lib.spng_status_string(st).decode()
        raise SpngError(st) if st != E_DEVICE else RuntimeError(f"libspng_mi355: {msg}")


def _cbuf(data):
    """`data` (None: nothing) as a ctypes byte array for a host-pointer entry: one zero byte where it is empty, for ctypes cannot point at
    an array of length 0"""
    data = b"" if data is None else bytes(data)
    return (ctypes.c_uint8 * max(len(data), 1)).from_buffer_copy(data or b"\0")


def pick(v, i):
    """an argument of a batch call that holds one value, or one per array: the value for array i"""
    return v[i] if isinstance(v, (list, tuple)) else v


def census_wide_sort_launches(keys) -> int:
    """launches of the sort of a wide census that found `keys` keys (between its gather and its write): one that sorts the tiles,
    then per stage above a tile one per stride of at least a tile and one for the strides below"""
    np_, launches, k = 1, 1, 2 * CENSUS_WIDE_TILE
    while np_ < keys:
        np_ <<= 1
    while k <= np_:
        launches += (k // 2 // CENSUS_WIDE_TILE).bit_length() + 1
        k <<= 1
    return launches


def miss_bytes(miss, value_bytes) -> bytes:
    """the `miss` of a map as the value_bytes bytes of spng_map_desc.miss: an int (little-endian) or bytes of that length"""
    b = bytes(miss) if isinstance(miss, (bytes, bytearray)) else int(miss).to_bytes(value_bytes, "little")
    if len(b) != value_bytes:
        raise ValueError("a miss value of value_bytes bytes is needed")
    return b


def pixel_bytes(layout, bits) -> int:
    """bytes of one RGBA<T> / VA<T> / T pixel, T of `bits` bits"""
    return (4, 2, 1)[layout] * (bits // 8)


# ---- indexers and deindexers as tables -------------------------------------------------------------
def palette_entries(palette):
    """bytes of (r, g, b, a) quadruplets -> the list of tuples an indexer / deindexer of the reference is created with"""
    p = bytes(palette or b"")
    return [tuple(p[i:i + 4]) for i in range(0, len(p) - len(p) % 4, 4)]


def key_aggregate(key: int, layout: int):
    """the UInt8 aggregate the reference hands to an indexer for a pixel whose key is `key`: (r, g, b, a), (v, a) or v"""
    if layout == TARGET_RGBA:
        return (key & 255, key >> 8 & 255, key >> 16 & 255, key >> 24 & 255)
    if layout == TARGET_VA:
        return (key & 255, key >> 8 & 255)
    return key & 255


def tabulate_indexer(index, keys, layout) -> bytes:
    """index: the closure an indexer made for a palette; keys: the pixel keys to evaluate it on -> one index byte per key.  An index
    outside 0 ... 255 raises, where Swift's UInt8(_:) traps (PNG.RGBA.swift:421)."""
    out = bytearray(len(keys))
    for j, k in enumerate(keys):
        i = int(index(key_aggregate(int(k), layout)))
        if not 0 <= i <= 255:
            raise OverflowError(f"indexer returned {i} for {key_aggregate(int(k), layout)}: not representable in UInt8")
        out[j] = i
    return bytes(out)


def tabulate_deindexer(dereference, layout=TARGET_RGBA) -> bytes:
    """dereference: the closure a deindexer made for a palette ((Int) -> (r, g, b, a) | (v, a) | v) -> the 256 x (r, g, b, a)
    table spng_unpack_desc.d_palette takes: a VA target reads the r and a slots, a scalar target the r slot."""
    out = bytearray(1024)
    for i in range(256):
        v = dereference(i)
        if layout == TARGET_RGBA:
            q = tuple(v)
        elif layout == TARGET_VA:
            q = (v[0], v[0], v[0], v[1])
        else:
            q = (v, v, v, 255)
        if len(q) != 4 or not all(0 <= int(x) <= 255 for x in q):
            raise OverflowError(f"deindexer returned {v!r} for {i}: UInt8 components are needed")
        out[4 * i:4 * i + 4] = bytes(int(x) for x in q)
    return bytes(out)


class Session:
    """One spng_ctx: a device, a HIP stream and its workspaces (re-entrant per handle)."""

    def __init__(self, device: int = 0, use_torch_stream: bool = True):
        import torch
        if not torch.cuda.is_available():
            raise RuntimeError("swift_png_amd needs an MI355X (gfx950); no HIP device is visible and there is "
                               "no CPU fallback")
        self.torch = torch
        self.lib = load_library()
        self.device = device
        self.tdev = torch.device("cuda", device)
        handle = ctypes.c_void_p()
        stream = None
        if use_torch_stream:
            with torch.cuda.device(device):
                stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        _check(self.lib, self.lib.spng_create(device, stream, ctypes.byref(handle)))
        self.ctx = handle

    def close(self):
        if self.ctx:
            self.lib.spng_destroy(self.ctx)
            self.ctx = None

    # -- plumbing -------------------------------------------------------------------------------
    def sync(self):
        _check(self.lib, self.lib.spng_sync(self.ctx))

    def configure(self, key, value):
        _check(self.lib, self.lib.spng_configure(self.ctx, key, int(value)))

    def profile(self, enable=True):
        _check(self.lib, self.lib.spng_profile(self.ctx, int(enable)))

    def trim(self):
        """gives the context's scratch (token pool, deflate slab ...) back to the device"""
        _check(self.lib, self.lib.spng_trim(self.ctx))

    def copy_ceiling(self, nbytes=8 << 30, pattern=0, repeats=5):
        """GB/s (read + write) of the library's own copy kernel between two buffers of nbytes: the measured ceiling next to the
        8 TB/s spec peak (pattern 0), or the bandwidth of the scanline kernel's former access pattern (pattern 1)"""
        t = self.torch
        a = t.zeros(nbytes // 8, dtype=t.int64, device=self.tdev)
        b = t.empty(nbytes // 8, dtype=t.int64, device=self.tdev)
        ms = ctypes.c_double(0)
        _check(self.lib, self.lib.spng_copy_ceiling(self.ctx, b.data_ptr(), a.data_ptr(), nbytes, pattern, repeats, ctypes.byref(ms)))
        del a, b
        return 2 * nbytes / (ms.value * 1e-3) / 1e9, ms.value

    def profile_get(self, kernel):
        ms, n = ctypes.c_double(0), ctypes.c_uint64(0)
        _check(self.lib, self.lib.spng_profile_get(self.ctx, kernel, ctypes.byref(ms), ctypes.byref(n)))
        return ms.value, n.value

    def token_stats(self):
        """(bytes of token pages, DEFLATE blocks, ran dry) of the most recent parallel-inflate call read back."""
        b, k, d = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_int32(0)
        _check(self.lib, self.lib.spng_token_stats(self.ctx, ctypes.byref(b), ctypes.byref(k), ctypes.byref(d)))
        return b.value, k.value, bool(d.value)

    def cut_stats(self):
        """(cut segments tried, cuts joined to the chain, streams decoded again without cuts) of the most recent parallel-inflate call."""
        t, j, r = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
        _check(self.lib, self.lib.spng_cut_stats(self.ctx, ctypes.byref(t), ctypes.byref(j), ctypes.byref(r)))
        return t.value, j.value, r.value

    def to_device(self, data):
        t = self.torch
        if isinstance(data, (bytes, bytearray, memoryview)):
            if len(data) == 0:
                return t.empty(0, dtype=t.uint8, device=self.tdev)
            return t.frombuffer(bytearray(data), dtype=t.uint8).to(self.tdev)
        return t.as_tensor(data, dtype=t.uint8).to(self.tdev)

    def empty(self, n):
        return self.torch.empty(max(int(n), 1), dtype=self.torch.uint8, device=self.tdev)

    @staticmethod
    def _ptr(tensor):
        return ctypes.c_void_p(tensor.data_ptr() if tensor is not None and tensor.numel() else None)

    # -- batch entry points (device tensors in, device tensors out) ------------------------------
    def inflate_batch(self, streams, caps, fmt=FORMAT_ZLIB):
        """streams: list of uint8 device tensors; caps: output capacities.
        -> (list of output tensors, list[Result])"""
        n = len(streams)
        outs = [self.empty(c) for c in caps]
        descs = (StreamDesc * n)()
        for i, (s, o, c) in enumerate(zip(streams, outs, caps)):
            descs[i] = StreamDesc(self._ptr(s), s.numel(), self._ptr(o), int(c), pick(fmt, i), 0)
        res = (Result * n)()
        _check(self.lib, self.lib.spng_inflate_batch(self.ctx, descs, n, None, res))
        return outs, list(res)

    def inflate_resume(self, src, src_len, dst, fmt=FORMAT_ZLIB, state=(0, 0, 0, 0)):
        """One push of a stream that arrives in pieces (spng_inflate_resume_batch): src / dst are device tensors that
        hold ALL compressed bytes so far (src_len of them) / the output so far; state is what the previous call
        returned: four words -- {header bit of the block the input ended in, bytes in front of it, first bit inside it that is
        still to decode (0: its header), bytes in front of that} (a pair is taken as a state at a block boundary).
        -> (Result, next state)"""
        desc = (StreamDesc * 1)(StreamDesc(self._ptr(src), int(src_len), self._ptr(dst), dst.numel(), fmt, 0))
        state = tuple(state) + (0, 0) * (len(state) == 2)
        st = (ctypes.c_uint64 * 4)(*[int(v) for v in state])
        res = (Result * 1)()
        _check(self.lib, self.lib.spng_inflate_resume_batch(self.ctx, desc, st, 1, None, res))
        r = res[0]
        if r.status == NEED_MORE_INPUT:
            tok = int(r.consumed)
            return r, (int(r.aux[0]), int(r.aux[1]), tok, int(r.written) if tok else 0)
        return r, tuple(state)

    def unfilter_resume(self, desc, work, prev_len, now_len):
        """The scanlines of one image that became complete between prev_len and now_len inflated bytes are defiltered and
        assigned (spng_unfilter_resume_batch); work: device scratch of the size of the scanline buffer (interlaced and
        sub-byte images), or None.  -> Result (written = scanline bytes defiltered by this call)"""
        arr = (ImageDesc * 1)(desc)
        wp = (ctypes.c_void_p * 1)(self._ptr(work) if work is not None else None)
        prev, now = (ctypes.c_uint64 * 1)(int(prev_len)), (ctypes.c_uint64 * 1)(int(now_len))
        res = (Result * 1)()
        _check(self.lib, self.lib.spng_unfilter_resume_batch(self.ctx, arr, wp, prev, now, 1, None, res))
        return res[0]

    def image_desc(self, idat, rows, storage, w, h, depth, channels, interlaced, fmt=FORMAT_ZLIB, rows_cap=None):
        return ImageDesc(self._ptr(idat), idat.numel() if idat is not None else 0, self._ptr(rows),
                         int(rows_cap if rows_cap is not None else rows.numel()), self._ptr(storage),
                         w, h, depth, channels, int(bool(interlaced)), fmt, 0)

    def decode_batch(self, descs, wait=True):
        """PNG.Context.push for a batch.  wait=True: -> list[Result]; wait=False: results stay on the
        device (fetch_results) and the call returns as soon as the kernels are enqueued."""
        n = len(descs)
        arr = descs if isinstance(descs, ctypes.Array) else (ImageDesc * n)(*descs)
        if wait:
            res = (Result * n)()
            _check(self.lib, self.lib.spng_decode_batch(self.ctx, arr, n, None, res))
            return list(res)
        if getattr(self, "_dres", None) is None or self._dres.numel() < n * ctypes.sizeof(Result):
            self._dres = self.empty(n * ctypes.sizeof(Result))
        _check(self.lib, self.lib.spng_decode_batch(self.ctx, arr, n, self._ptr(self._dres), None))
        return None

    def fetch_results(self, n):
        raw = bytes(self._dres[:n * ctypes.sizeof(Result)].cpu().numpy())
        return list((Result * n).from_buffer_copy(raw))

    def unfilter_batch(self, descs, rows_len=None):
        n = len(descs)
        arr = (ImageDesc * n)(*descs)
        res = (Result * n)()
        dl = None
        if rows_len is not None:
            dl = self.torch.tensor(list(rows_len), dtype=self.torch.int64, device=self.tdev)
        _check(self.lib, self.lib.spng_unfilter_batch(self.ctx, arr, n, self._ptr(dl) if dl is not None else None,
                                                      None, res))
        return list(res)

    def filter_batch(self, descs):
        n = len(descs)
        arr = (ImageDesc * n)(*descs)
        res = (Result * n)()
        _check(self.lib, self.lib.spng_filter_batch(self.ctx, arr, n, None, res))
        return list(res)

    # -- host-buffer conveniences ------------------------------------------------------------------
    def inflate(self, data: bytes, fmt=FORMAT_ZLIB, cap=None):
        """Whole-stream LZ77.Inflator: -> (status, bytes, consumed, aux)"""
        cap = int(cap if cap is not None else max(1 << 16, 1100 * len(data)))
        dst = (ctypes.c_uint8 * max(cap, 1))()
        res = Result()
        _check(self.lib, self.lib.spng_inflate(self.ctx, _cbuf(data), len(data), fmt, dst, cap, ctypes.byref(res)))
        return res.status, bytes(dst[:res.written]), res.consumed, (res.aux[0], res.aux[1])

    def decode(self, idat: bytes, w, h, depth, channels, interlaced, fmt=FORMAT_ZLIB, storage=None):
        """PNG.Context.push over the concatenated IDAT payload: -> (status, storage bytes, aux)"""
        s = storage_size(w, h, depth, channels)
        buf = (ctypes.c_uint8 * max(s, 1))()
        if storage is not None:
            ctypes.memmove(buf, bytes(storage), s)
        res = Result()
        _check(self.lib, self.lib.spng_decode(self.ctx, _cbuf(idat), len(idat), fmt, w, h, depth, channels,
                                              int(bool(interlaced)), buf, ctypes.byref(res)))
        return res.status, bytes(buf[:s]), (res.aux[0], res.aux[1])

    def unfilter(self, rows: bytes, w, h, depth, channels, interlaced, storage=None):
        s = storage_size(w, h, depth, channels)
        buf = (ctypes.c_uint8 * max(s, 1))()
        if storage is not None:
            ctypes.memmove(buf, bytes(storage), s)
        res = Result()
        _check(self.lib, self.lib.spng_unfilter(self.ctx, _cbuf(rows), len(rows), w, h, depth, channels,
                                                int(bool(interlaced)), buf, ctypes.byref(res)))
        return res.status, bytes(buf[:s])

    def filter(self, storage: bytes, w, h, depth, channels, interlaced) -> bytes:
        u = inflated_size(w, h, depth, channels, interlaced)
        dst = (ctypes.c_uint8 * max(u, 1))()
        res = Result()
        _check(self.lib, self.lib.spng_filter(self.ctx, _cbuf(storage), w, h, depth, channels, int(bool(interlaced)), dst,
                                              ctypes.byref(res)))
        return bytes(dst[:u])

    def lex_batch(self, files):
        """files: list of PNG file bytes -> (list[Lexed], list of concatenated IDAT payloads as bytes).
        The lexing half of PNG.Image.decompress(stream:) for files resident in HBM."""
        n = len(files)
        d_png = [self.to_device(f) for f in files]
        d_idat = [self.empty(len(f)) for f in files]
        descs = (FileDesc * n)()
        for i, (f, a, b) in enumerate(zip(files, d_png, d_idat)):
            descs[i] = FileDesc(self._ptr(a), len(f), self._ptr(b), len(f))
        infos = (Lexed * n)()
        _check(self.lib, self.lib.spng_lex_batch(self.ctx, descs, n, None, infos))
        return list(infos), [bytes(b[:r.idat_len].cpu().numpy()) for b, r in zip(d_idat, infos)]

    def lex_dir_batch(self, files, caps=None, d_png=None, device_idat=False):
        """lex_batch with a chunk directory (spng_lex_dir_batch).  files: list of PNG file bytes; caps: entries of room per file
        (None: what a file of its length can hold at most); d_png: the files as device tensors, if they are there already.
        -> (list[Lexed], list of IDAT payloads -- bytes, or with device_idat the device tensors they were written to --, list of
        list[ChunkEntry]: the first min(chunks, cap) entries of each file)"""
        n = len(files)
        d_png = d_png or [self.to_device(f) for f in files]
        d_idat = [self.empty(len(f)) for f in files]
        caps = [len(f) // 12 for f in files] if caps is None else [int(c) for c in caps]
        sz = ctypes.sizeof(ChunkEntry)
        d_ent = [self.torch.full((max(c, 1) * sz,), 0xEE, dtype=self.torch.uint8, device=self.tdev) for c in caps]
        descs, dirs = (FileDesc * max(n, 1))(), (ChunkDir * max(n, 1))()
        for i, (f, a, b) in enumerate(zip(files, d_png, d_idat)):
            descs[i] = FileDesc(self._ptr(a), len(f), self._ptr(b), len(f))
            dirs[i] = ChunkDir(d_ent[i].data_ptr() if caps[i] else None, caps[i], 0)
        infos = (Lexed * max(n, 1))()
        _check(self.lib, self.lib.spng_lex_dir_batch(self.ctx, descs, dirs, n, None, infos))
        entries = []
        for r, c, e in zip(infos, caps, d_ent):
            k = min(r.chunks, c)
            raw = bytes(e[:k * sz].cpu().numpy())
            entries.append(list((ChunkEntry * k).from_buffer_copy(raw)))
        idats = d_idat if device_idat else [bytes(b[:r.idat_len].cpu().numpy()) for b, r in zip(d_idat, infos)]
        return list(infos)[:n], idats, entries

    def lex_parse_batch(self, files, caps=None, d_png=None):
        """lex_dir_batch with the typed chunks: spng_lex_dir_batch with its infos left on the device, and parse_dir_batch directly
        behind it -- nothing waits in between.  -> (list[Lexed], list of list[ChunkEntry], list of list[ChunkValue], list[Parsed],
        d_png, d_idat: the device tensors of the files and of their IDAT payloads)"""
        t = self.torch
        n = len(files)
        d_png = d_png or [self.to_device(f) for f in files]
        d_idat = [self.empty(len(f)) for f in files]
        caps = [len(f) // 12 for f in files] if caps is None else [int(c) for c in caps]
        esz = ctypes.sizeof(ChunkEntry)
        d_ent = [t.full((max(c, 1) * esz,), 0xEE, dtype=t.uint8, device=self.tdev) for c in caps]
        d_infos = t.zeros(max(n, 1) * ctypes.sizeof(Lexed), dtype=t.uint8, device=self.tdev)
        descs, dirs = (FileDesc * max(n, 1))(), (ChunkDir * max(n, 1))()
        for i, (f, a, b) in enumerate(zip(files, d_png, d_idat)):
            descs[i] = FileDesc(self._ptr(a), len(f), self._ptr(b), len(f))
            dirs[i] = ChunkDir(d_ent[i].data_ptr() if caps[i] else None, caps[i], 0)
        _check(self.lib, self.lib.spng_lex_dir_batch(self.ctx, descs, dirs, n, d_infos.data_ptr(), None))
        values, parsed = self.parse_dir_batch(files, d_png, dirs, d_infos)
        infos = list((Lexed * max(n, 1)).from_buffer_copy(d_infos.cpu().numpy().tobytes()))[:n]
        entries = [list((ChunkEntry * len(v)).from_buffer_copy(e[:len(v) * esz].cpu().numpy().tobytes())) for e, v in zip(d_ent, values)]
        return infos, entries, values, parsed, d_png, d_idat

    def parse_dir_batch(self, files, d_png, dirs, d_infos):
        """spng_parse_dir_batch behind a spng_lex_dir_batch whose results are still on the device.  files: list of PNG file bytes (their
        lengths are what counts); d_png: the files as device tensors; dirs: the (ChunkDir * n) array the directory was made with;
        d_infos: the device tensor its infos went to.  -> (list of list[ChunkValue] -- the first min(chunks, cap) records of each
        file --, list[Parsed])"""
        t = self.torch
        n = len(files)
        vsz = ctypes.sizeof(ChunkValue)
        d_val = [t.full((max(dirs[i].cap, 1) * vsz,), 0xEE, dtype=t.uint8, device=self.tdev) for i in range(n)]
        descs, vals = (FileDesc * max(n, 1))(), (ctypes.c_void_p * max(n, 1))()
        for i, (f, a) in enumerate(zip(files, d_png)):
            descs[i] = FileDesc(self._ptr(a), len(f), None, 0)
            vals[i] = d_val[i].data_ptr() if dirs[i].cap else None
        parsed = (Parsed * max(n, 1))()
        _check(self.lib, self.lib.spng_parse_dir_batch(self.ctx, descs, dirs, self._ptr(d_infos), vals, n, None, parsed))
        infos = (Lexed * max(n, 1)).from_buffer_copy(d_infos.cpu().numpy().tobytes())
        out = []
        for i in range(n):
            k = min(infos[i].chunks, dirs[i].cap)
            out.append(list((ChunkValue * k).from_buffer_copy(d_val[i][:k * vsz].cpu().numpy().tobytes())))
        return out, list(parsed)[:n]

    def text_batch(self, texts, op, out_caps=None):
        """spng_text_batch over device tensors (or bytes, which are uploaded).  op: TEXT_LATIN1_TO_UTF8 / TEXT_CHECK_UTF8, one or a list;
        out_caps: capacities of the outputs (None: twice the input, which always fits).  -> (list of output tensors -- None for a
        check --, list[Result])"""
        n = len(texts)
        ts = [self.to_device(t) if isinstance(t, (bytes, bytearray, memoryview)) else t for t in texts]
        outs, descs = [], (TextDesc * max(n, 1))()
        for i, t in enumerate(ts):
            o = pick(op, i)
            cap = 0 if o == TEXT_CHECK_UTF8 else 2 * t.numel() if out_caps is None else int(out_caps[i])
            outs.append(None if o == TEXT_CHECK_UTF8 else self.empty(cap))
            descs[i] = TextDesc(self._ptr(t), t.numel(), self._ptr(outs[-1]) if outs[-1] is not None else None, cap, o, (ctypes.c_uint8 * 7)())
        res = (Result * max(n, 1))()
        _check(self.lib, self.lib.spng_text_batch(self.ctx, descs, n, None, res))
        return outs, list(res)[:n]

    def lex_states(self, count=1):
        """`count` states for lex_resume_batch: spng_lex_state_bytes() zero bytes of device memory each, one per file, kept by the
        caller between the pushes of that file"""
        t = self.torch
        return [t.zeros(int(self.lib.spng_lex_state_bytes()), dtype=t.uint8, device=self.tdev) for _ in range(count)]

    def lex_resume_batch(self, files, states):
        """One push of files that arrive in pieces (spng_lex_resume_batch).  files: per file (d_png, length, d_idat) -- device tensors
        with ALL bytes of the file so far (`length` of them) and the IDAT payloads so far (its size is idat_cap); states: per file
        a tensor of lex_states(), or None (that file answers SPNG_E_ARGUMENT).  -> list[Lexed]: what lex_batch reports for the
        same prefixes as whole files; d_idat[:idat_len] holds the verified payloads."""
        n = len(files)
        if n == 0:
            _check(self.lib, self.lib.spng_lex_resume_batch(self.ctx, None, None, 0, None, None))
            return []
        descs = (FileDesc * n)()
        for i, (png, length, idat) in enumerate(files):
            descs[i] = FileDesc(self._ptr(png), int(length), self._ptr(idat), idat.numel() if idat is not None else 0)
        sp = (ctypes.c_void_p * n)(*[s.data_ptr() if s is not None else None for s in states])
        infos = (Lexed * n)()
        _check(self.lib, self.lib.spng_lex_resume_batch(self.ctx, descs, sp, n, None, infos))
        return list(infos)

    def lex_resume_stats(self):
        """(bytes summed by the CRC, IDAT bytes copied, chunk headers walked) of the most recent lex_resume_batch, over its files"""
        a, b, c = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
        _check(self.lib, self.lib.spng_lex_resume_stats(self.ctx, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)))
        return a.value, b.value, c.value

    def write_idat(self, stream: bytes, chunk_bytes: int) -> bytes:
        """The IDAT chunks (length, type, data, CRC-32 each) of a zlib stream cut every chunk_bytes bytes."""
        pieces = -(-len(stream) // chunk_bytes) if stream else 0
        cap = len(stream) + 12 * pieces
        src, dst = self.to_device(stream), self.empty(cap)
        d = (ChunkingDesc * 1)(ChunkingDesc(self._ptr(src), len(stream), self._ptr(dst), cap, chunk_bytes))
        res = (Result * 1)()
        _check(self.lib, self.lib.spng_write_idat_batch(self.ctx, d, 1, None, res))
        raise_for(res[0].status)
        return bytes(dst[:res[0].written].cpu().numpy())

    def write_file_batch(self, descs, d_results=None, wait=True):
        """spng_write_file_batch over PngDesc records whose device fields are filled in.  wait: -> list[Result]; else the results stay
        in the device tensor d_results and the call returns once the kernels are enqueued"""
        n = len(descs)
        arr = descs if isinstance(descs, ctypes.Array) else (PngDesc * n)(*descs)
        res = (Result * n)() if wait else None
        _check(self.lib, self.lib.spng_write_file_batch(self.ctx, arr, n, self._ptr(d_results) if d_results is not None else None, res))
        return list(res) if wait else None

    def write_file(self, stream: bytes, size, depth, channels, chunk_bytes=65544, **fmt) -> bytes:
        """The PNG file around a zlib stream: signature, the head PNG.Image.compress(stream:level:hint:) writes for the format (png_desc:
        indexed, bgr, interlaced, palette, key, fill, before, after), the stream in IDAT chunks of chunk_bytes, IEND."""
        d, keep = png_desc(size, depth, channels, chunk_bytes=chunk_bytes, **fmt)
        cap = int(self.lib.spng_file_bound(ctypes.byref(d), len(stream)))
        src, dst = self.to_device(stream), self.empty(cap)
        d.d_stream, d.stream_len, d.d_out, d.out_cap = src.data_ptr() if len(stream) else dst.data_ptr(), len(stream), dst.data_ptr(), cap
        (res,) = self.write_file_batch([d])
        raise_for(res.status, (res.aux[0], res.aux[1]))
        if res.status != DONE:
            raise SpngError(res.status)
        return bytes(dst[:res.written].cpu().numpy())

    def compress_batch(self, images, level=9):
        """PNG.Image.compress(stream:level:hint:) from storage for a batch, one call of spng_compress_batch: images: dicts of
        storage (bytes, or a uint8 device tensor: the pixels stay on the device), size, depth, channels and what png_desc takes (indexed, bgr, interlaced, palette, key, fill, before, after,
        chunk_bytes).  -> list of file bytes"""
        n = len(images)
        idescs, fdescs, keep, outs = (ImageDesc * n)(), (PngDesc * n)(), [], []
        for i, im in enumerate(images):
            im = dict(im)
            storage, size, depth, channels = im.pop("storage"), im.pop("size"), im.pop("depth"), im.pop("channels")
            interlaced, bgr = bool(im.get("interlaced", False)), bool(im.get("bgr", False))
            u = inflated_size(size[0], size[1], depth, channels, interlaced)
            bound = int(self.lib.spng_deflate_bound(u))
            d, k = png_desc(size, depth, channels, **im)
            d_storage = storage if self.torch.is_tensor(storage) else self.to_device(bytes(storage))
            d_rows, d_idat = self.empty(u), self.empty(bound)
            cap = int(self.lib.spng_file_bound(ctypes.byref(d), bound))
            d_out = self.empty(cap)
            d.d_out, d.out_cap = d_out.data_ptr(), cap
            idescs[i] = self.image_desc(d_idat, d_rows, d_storage, size[0], size[1], depth, channels, interlaced, FORMAT_IOS if bgr else FORMAT_ZLIB,
                                        rows_cap=u)
            fdescs[i] = d
            keep += [k, d_storage, d_rows, d_idat]
            outs.append(d_out)
        res = (Result * n)()
        _check(self.lib, self.lib.spng_compress_batch(self.ctx, idescs, fdescs, int(level), n, None, res))
        for r in res:
            raise_for(r.status, (r.aux[0], r.aux[1]))
            if r.status != DONE:
                raise SpngError(r.status)
        return [bytes(o[:r.written].cpu().numpy()) for o, r in zip(outs, res)]

    def compress(self, storage: bytes, size, depth, channels, level=9, **fmt) -> bytes:
        """One image: storage in, the bytes of its PNG file out"""
        return self.compress_batch([dict(fmt, storage=storage, size=size, depth=depth, channels=channels)], level)[0]

    def crc32(self, data: bytes) -> int:
        out = ctypes.c_uint32(0)
        _check(self.lib, self.lib.spng_crc32(self.ctx, _cbuf(data), len(data), ctypes.byref(out)))
        return out.value

    def unpack(self, storage: bytes, w, h, depth, channels, indexed=False, bgr=False, target=16, palette=None, key=None,
               layout=0, premultiply=0, deindexer=None):
        """PNG.Image.unpack(as: PNG.RGBA<UInt8 / UInt16>.self) (layout = TARGET_VA: PNG.VA<T>): -> bytes of r, g, b, a
        (v, a) per pixel (host order).  palette: bytes of (r, g, b, a) quadruplets (PLTE with the tRNS alphas folded in);
        key: tRNS chroma key; premultiply: 0, PREMULTIPLY (.premultiplied) or PREMULTIPLY_AS_U8 (.premultiplied(as: UInt8.self)).
        deindexer (indexed formats): shaped like the reference's (unpack(as:deindexer:), PNG.Image.swift:836-933): deindexer(palette)
        returns a function of the index; it is tabulated over 0 ... 255 into the palette the kernel dereferences."""
        if deindexer is not None:
            if not indexed:
                raise ValueError("a deindexer needs an indexed format")
            palette = tabulate_deindexer(deindexer(palette_entries(palette)), layout)
        n = w * h * pixel_bytes(layout, target)
        out = (ctypes.c_uint8 * max(n, 1))()
        k = (ctypes.c_uint16 * 3)(*(list(key) + [0, 0, 0])[:3]) if key is not None else None
        _check(self.lib, self.lib.spng_unpack_as(self.ctx, _cbuf(storage), w, h, depth, channels, int(bool(indexed)), int(bool(bgr)), target,
                                                 int(layout), int(premultiply), _cbuf(palette) if palette else None, len(palette or b"") // 4, k, out))
        return bytes(out[:n])

    def pack(self, pixels: bytes, w, h, depth, channels, indexed=False, bgr=False, source=16, palette=None, layout=0,
             premultiply=0, indexer=None) -> bytes:
        """PNG.Image(packing:size:layout:).storage for [PNG.RGBA<T>] (layout TARGET_RGBA), [PNG.VA<T>] (TARGET_VA) or [T]
        (TARGET_SCALAR), T = UInt8 / UInt16 (`source` bits), with the default indexer: pixels = bytes of r, g, b, a | v, a | v per
        pixel (host order) -> storage bytes.  palette: bytes of (r, g, b, a) quadruplets.  premultiply: 0, PREMULTIPLY or
        PREMULTIPLY_AS_U8 -- pack(pixels.map(\\.premultiplied)) in one pass (spng_pack_desc.premultiply).
        indexer (indexed8 only): shaped like the reference's (init(packing:size:layout:metadata:indexer:), PNG.Image.swift:935-996):
        indexer(palette) returns a function of the UInt8 aggregate -- (r, g, b, a), (v, a) or v -- that returns the index.  Scalar
        and VA layouts tabulate it over all 256 / 65536 aggregates; the RGBA layout asks the device for the distinct colours of the
        pixels (census, at most 65536: SpngError(E_OUTPUT_CAPACITY) above) and calls it once per colour.  Images of more colours:
        map_colours with dtype uint8, whose function takes all keys at once."""
        if indexer is not None:
            if not indexed or depth != 8:
                raise ValueError("an indexer needs the indexed8 format")
            if len(pixels) != w * h * pixel_bytes(layout, source):
                raise ValueError("pixel array `count` must be equal to `size.x * size.y`")
            index = indexer(palette_entries(palette))
            if layout == TARGET_RGBA:
                keys, _ = self.census(pixels, source, layout, cap=65536, premultiply=premultiply)
            else:
                keys = range(256 if layout == TARGET_SCALAR else 65536)
            keys = list(keys)
            storage, _ = self.pack_indexed(pixels, w, h, source, layout, keys, tabulate_indexer(index, keys, layout),
                                           premultiply=premultiply)
            return storage
        if len(pixels) != w * h * pixel_bytes(layout, source):
            raise ValueError("pixel array `count` must be equal to `size.x * size.y`")
        n = self.lib.spng_storage_size(w, h, depth, channels)
        if premultiply:
            # (spng_pack_as has no such argument: the batch entry on device buffers)
            d_px, d_sto = self.to_device(bytes(pixels)), self.empty(n)
            d_pal = self.to_device(bytes(palette)) if palette else None
            desc = (PackDesc * 1)(PackDesc(self._ptr(d_px), self._ptr(d_sto), self._ptr(d_pal), w, h, len(palette or b"") // 4, depth,
                                           channels, int(bool(indexed)), int(bool(bgr)), source, int(layout), int(premultiply)))
            _check(self.lib, self.lib.spng_pack_batch(self.ctx, desc, 1))
            self.sync()
            return bytes(d_sto[:n].cpu().numpy())
        out = (ctypes.c_uint8 * max(n, 1))()
        _check(self.lib, self.lib.spng_pack_as(self.ctx, _cbuf(pixels), w, h, depth, channels, int(bool(indexed)), int(bool(bgr)), source,
                                               int(layout), _cbuf(palette) if palette else None, len(palette or b"") // 4, out))
        return bytes(out[:n])

    def census_batch(self, arrays, bits, layout, cap=256, premultiply=0, counts=True, outs=None, wide=False):
        """spng_census_batch (wide: spng_census_wide_batch, see census_wide_batch) on device tensors: every tensor of `arrays` holds whole RGBA<T> / VA<T> / T pixels (T of `bits`
        bits; layout, cap and premultiply: one value, or one per array).  -> (list of (keys, counts) device tensors -- int32 /
        int64 bit patterns of the uint32 keys and uint64 counts, `cap` long, valid up to Result.written; or the (keys, counts) pairs of
        `outs`, of at least 4 * cap / 8 * cap bytes --, list[Result]).  Like every batch entry it runs on the context's stream: tensors
        that torch kernels are still writing have to be waited for first."""
        n = len(arrays)
        t = self.torch
        descs = (CensusDesc * max(n, 1))()
        given, outs = outs, []
        for i, a in enumerate(arrays):
            lay, cp = pick(layout, i), pick(cap, i)
            nbytes, per = a.numel() * a.element_size(), pixel_bytes(lay, bits)
            if nbytes % per:
                raise ValueError("an array of whole pixels is needed")
            room = min(cp, max(nbytes // per, 1)) if wide else cp           # (wide: no more keys than pixels)
            if given is not None:
                k, c = given[i]
                if k.numel() * k.element_size() < 4 * room or (c is not None and c.numel() * c.element_size() < 8 * room):
                    raise ValueError("outputs of cap keys and cap counts are needed")
            else:
                k = t.empty(max(room, 1), dtype=t.int32, device=self.tdev)
                c = t.empty(max(room, 1), dtype=t.int64, device=self.tdev) if counts else None
            outs.append((k, c))
            descs[i] = CensusDesc(self._ptr(a), nbytes // per, self._ptr(k), self._ptr(c), cp, bits, lay, pick(premultiply, i))
        res = (Result * max(n, 1))()
        entry = self.lib.spng_census_wide_batch if wide else self.lib.spng_census_batch
        _check(self.lib, entry(self.ctx, descs, n, None, res))
        return outs, list(res)[:n]

    def census_wide_batch(self, arrays, bits, layout, cap=CENSUS_WIDE_CAP, premultiply=0, counts=True, outs=None):
        """spng_census_wide_batch on device tensors: census_batch with cap up to CENSUS_WIDE_CAP (2^24).  The outputs hold
        min(cap, pixels) keys and counts -- an array has no more keys than pixels, so the default cap asks for "all of them".  The
        call waits once, for the counting kernel."""
        return self.census_batch(arrays, bits, layout, cap, premultiply, counts, outs, wide=True)

    def census_wide(self, pixels: bytes, bits, layout, cap=CENSUS_WIDE_CAP, premultiply=0):
        """census without the ceiling of 65536 keys: -> (keys, counts) as numpy arrays (uint32 ascending, uint64).  More than `cap`
        (at most 2^24) distinct keys raise SpngError(E_OUTPUT_CAPACITY)."""
        import numpy as np
        per = pixel_bytes(layout, bits)
        if len(pixels) % per:
            raise ValueError("whole pixels are needed")
        n = len(pixels) // per
        room = max(min(cap, n), 1)
        keys, counts = np.empty(room, dtype=np.uint32), np.empty(room, dtype=np.uint64)
        res = Result()
        _check(self.lib, self.lib.spng_census_wide(self.ctx, _cbuf(pixels), n, bits, int(layout), int(premultiply), cap, keys.ctypes.data,
                                                   counts.ctypes.data, ctypes.byref(res)))
        raise_for(res.status)
        return keys[:res.written], counts[:res.written]

    def map_batch(self, arrays, source, layout, keys, values, value_bytes, miss=0, premultiply=0, outs=None):
        """spng_map_batch on device tensors: every pixel of arrays[i] (whole RGBA<T> / VA<T> / T pixels, T of `source` bits) stores
        values[i][j] -- items of value_bytes (1, 2, 4 or 8; one value, or one per array) bytes -- where keys[i][j] (uint32, ascending
        and distinct, int32 bit patterns) is its key, and `miss` (an int or value_bytes bytes) where none is.  -> (list of uint8 output
        tensors of pixels * value_bytes bytes, or `outs`; list[Result] with aux[0] = pixels that missed)"""
        n = len(arrays)
        descs = (MapDesc * max(n, 1))()
        given, outs = outs, []
        for i, a in enumerate(arrays):
            lay, vb = pick(layout, i), pick(value_bytes, i)
            nbytes, per = a.numel() * a.element_size(), pixel_bytes(lay, source)
            if nbytes % per:
                raise ValueError("an array of whole pixels is needed")
            o = given[i] if given is not None else self.empty(nbytes // per * vb)
            outs.append(o)
            k, v = keys[i], values[i]
            mc = k.numel() if k is not None else 0
            descs[i] = MapDesc(self._ptr(a), self._ptr(o), self._ptr(k) if mc else None, self._ptr(v) if mc else None, nbytes // per, mc,
                               source, lay, pick(premultiply, i), vb, (ctypes.c_uint8 * 8)(*miss_bytes(pick(miss, i), vb)))
        res = (Result * max(n, 1))()
        _check(self.lib, self.lib.spng_map_batch(self.ctx, descs, n, None, res))
        return outs, list(res)[:n]

    def map(self, pixels: bytes, source, layout, keys, values, miss=0, premultiply=0):
        """One value per pixel: values[j] -- a numpy array whose items have 1, 2, 4 or 8 bytes -- where keys[j] (ascending, distinct)
        is the pixel's key, `miss` (an int or bytes of one item) where none is.  -> (numpy array of values' dtype, pixels that missed)"""
        import numpy as np
        per = pixel_bytes(layout, source)
        if len(pixels) % per:
            raise ValueError("whole pixels are needed")
        values = np.ascontiguousarray(values)
        keys = np.ascontiguousarray(keys, dtype=np.uint32)
        vb = values.dtype.itemsize
        if vb not in (1, 2, 4, 8) or values.ndim != 1:
            raise ValueError("values of 1, 2, 4 or 8 bytes each are needed")
        if len(keys) != len(values):
            raise ValueError("one value per key is needed")
        n = len(pixels) // per
        out = np.empty(max(n, 1), dtype=values.dtype)
        res = Result()
        _check(self.lib, self.lib.spng_map(self.ctx, _cbuf(pixels), n, source, int(layout), int(premultiply), keys.ctypes.data if len(keys) else None,
                                           values.ctypes.data if len(keys) else None, len(keys), vb, _cbuf(miss_bytes(miss, vb)),
                                           out.ctypes.data, ctypes.byref(res)))
        raise_for(res.status)
        return out[:n], int(res.aux[0])

    def map_colours(self, pixels: bytes, bits, layout, fn, dtype, premultiply=0, miss=0):
        """Any pure function of a pixel's UInt8 aggregate, applied to every pixel on the device: an indexer closure
        (PNG.RGBA.swift:409-423, PNG.VA.swift:334-350, PNG.Image.swift:767-782) or a colour target of the caller's own
        (Snippets/PNG/CustomColor.swift), as a table.  A wide census (cap = min(pixels, 2^24)) finds the distinct keys; fn(keys) is
        called ONCE, with the ascending uint32 numpy array of them (r | g << 8 | b << 16 | a << 24, v | a << 8 or v), and returns
        an array of `dtype` -- 1, 2, 4 or 8 bytes per item, structured dtypes included --, one item per key; the map stores it for
        every pixel.  -> numpy array of dtype, one item per pixel.  With dtype uint8 this is pack(indexer=) for images of more than
        65536 colours (vectorised: a million Python calls is not an interface).  `miss` is never stored: every key is in the table."""
        import numpy as np
        dtype = np.dtype(dtype)
        if dtype.itemsize not in (1, 2, 4, 8):
            raise ValueError("a dtype of 1, 2, 4 or 8 bytes is needed")
        per = pixel_bytes(layout, bits)
        if len(pixels) % per:
            raise ValueError("whole pixels are needed")
        n = len(pixels) // per
        keys, _ = self.census_wide(pixels, bits, layout, cap=max(min(n, CENSUS_WIDE_CAP), 1), premultiply=premultiply)
        keys = np.asarray(keys, dtype=np.uint32)
        values = np.ascontiguousarray(np.asarray(fn(keys), dtype=dtype))
        if values.shape != keys.shape:
            raise ValueError("fn returns one item per key")
        out, _ = self.map(pixels, bits, layout, keys, values.view("V%d" % dtype.itemsize), miss=miss, premultiply=premultiply)
        return np.asarray(out).view(dtype)

    def census(self, pixels: bytes, bits, layout, cap=256, premultiply=0):
        """The distinct UInt8 aggregates ("keys": r | g << 8 | b << 16 | a << 24, v | a << 8 or v) of [PNG.RGBA<T>] / [PNG.VA<T>] /
        [T] as bytes (host order), ascending, and how many pixels have each: -> (list of keys, list of counts).  More than `cap`
        (at most 65536) distinct keys raise SpngError(E_OUTPUT_CAPACITY)."""
        per = pixel_bytes(layout, bits)
        if len(pixels) % per:
            raise ValueError("whole pixels are needed")
        keys, counts = (ctypes.c_uint32 * max(cap, 1))(), (ctypes.c_uint64 * max(cap, 1))()
        res = Result()
        _check(self.lib, self.lib.spng_census(self.ctx, _cbuf(pixels), len(pixels) // per, bits, int(layout), int(premultiply), cap, keys, counts,
                                              ctypes.byref(res)))
        raise_for(res.status)
        return list(keys[:res.written]), list(counts[:res.written])

    def pack_indexed_batch(self, arrays, sizes, source, layout, keys, indices, miss=0, premultiply=0, storages=None):
        """spng_pack_indexed_batch on device tensors: arrays[i] holds sizes[i] = (w, h) pixels; keys[i] (uint32, ascending and
        distinct, int32 bit patterns) and indices[i] (uint8) are its map, equally long.  -> (list of storage tensors, list[Result]
        with aux[0] = pixels that missed)"""
        n = len(arrays)
        descs = (PackIndexedDesc * max(n, 1))()
        outs = []
        for i, a in enumerate(arrays):
            w, h = sizes[i]
            o = storages[i] if storages is not None else self.empty(w * h)
            outs.append(o)
            k, ix = keys[i], indices[i]
            mc = ix.numel() if ix is not None else 0
            descs[i] = PackIndexedDesc(self._ptr(a), self._ptr(o), self._ptr(k) if mc else None, self._ptr(ix) if mc else None, w, h, mc,
                                       source, pick(layout, i), pick(premultiply, i), pick(miss, i))
        res = (Result * max(n, 1))()
        _check(self.lib, self.lib.spng_pack_indexed_batch(self.ctx, descs, n, None, res))
        return outs, list(res)[:n]

    def pack_indexed(self, pixels: bytes, w, h, source, layout, keys, indices, miss=0, premultiply=0):
        """One index byte per pixel: indices[j] where keys[j] (ascending, distinct) is the pixel's key, `miss` where none is.
        -> (storage bytes, pixels that missed)"""
        if len(pixels) != w * h * pixel_bytes(layout, source):
            raise ValueError("pixel array `count` must be equal to `size.x * size.y`")
        if len(keys) != len(indices):
            raise ValueError("one index per key is needed")
        k = (ctypes.c_uint32 * max(len(keys), 1))(*keys)
        ix = (ctypes.c_uint8 * max(len(indices), 1))(*bytes(indices))
        out = (ctypes.c_uint8 * max(w * h, 1))()
        res = Result()
        _check(self.lib, self.lib.spng_pack_indexed(self.ctx, _cbuf(pixels), w, h, source, int(layout), int(premultiply), k, ix, len(keys),
                                                    int(miss), out, ctypes.byref(res)))
        raise_for(res.status)
        return bytes(out[:w * h]), int(res.aux[0])

    def alpha_batch(self, arrays, bits, layout, op, outs=None):
        """spng_alpha_batch on device tensors: every tensor of `arrays` holds whole RGBA<T> / VA<T> pixels (T of `bits` bits)
        and is premultiplied or straightened (`op`: PREMULTIPLY ... STRAIGHTEN_AS_U8; one value, or one per array, like
        `layout`) into the tensor of `outs` at its place -- in place where outs is None.  -> list[Result] (aux[0]: components
        the reference would have trapped on, written as T.max)"""
        n = len(arrays)
        descs = (AlphaDesc * max(n, 1))()
        for i, t in enumerate(arrays):
            lay = pick(layout, i)
            o = outs[i] if outs is not None else t
            nbytes = t.numel() * t.element_size()
            per = (4, 2)[lay] * (bits // 8)
            if nbytes % per or o.numel() * o.element_size() < nbytes:
                raise ValueError("an array of whole pixels and an output of at least its size are needed")
            descs[i] = AlphaDesc(self._ptr(t), self._ptr(o), nbytes // per, bits, lay, pick(op, i))
        res = (Result * max(n, 1))()
        _check(self.lib, self.lib.spng_alpha_batch(self.ctx, descs, n, None, res))
        return list(res)[:n]

    def alpha(self, pixels: bytes, bits, layout, op):
        """pixels.map(\\.premultiplied) / .map(\\.straightened) and their (as: UInt8.self) forms for [PNG.RGBA<T>] / [PNG.VA<T>]
        as bytes (host order): -> (bytes, trapped components)"""
        per = (4, 2)[layout] * (bits // 8)
        if len(pixels) % per:
            raise ValueError("whole pixels are needed")
        out = (ctypes.c_uint8 * max(len(pixels), 1))()
        res = Result()
        _check(self.lib, self.lib.spng_alpha(self.ctx, _cbuf(pixels), len(pixels) // per, bits, int(layout), int(op), out, ctypes.byref(res)))
        return bytes(out[:len(pixels)]), int(res.aux[0])

    def hsva_batch(self, arrays, ops, outs=None):
        """spng_hsva_batch on device tensors: every tensor of `arrays` holds whole pixels -- RGBA<UInt8> for HSVA_FROM_RGBA8, HSVA
        ({uint32 h; uint16 s; uint8 v; uint8 a}, 8 bytes, aligned to 4) for HSVA_TO_RGBA8 and HSVA_TO_VA8 -- and is converted into
        the tensor of `outs` at its place (never in place: the element sizes differ), or into a new uint8 tensor where outs is
        None.  ops: one value, or one per array.  -> (list of output tensors, list[Result] with aux[0] = pixels the reference would
        have trapped on, written as (v, v, v, a))"""
        n = len(arrays)
        descs = (HsvaDesc * max(n, 1))()
        given, outs = outs, []
        for i, t in enumerate(arrays):
            op = pick(ops, i)
            if op not in _HSVA_BYTES:
                raise ValueError("op must be HSVA_FROM_RGBA8, HSVA_TO_RGBA8 or HSVA_TO_VA8")
            per_in, per_out = _HSVA_BYTES[op]
            nbytes = t.numel() * t.element_size()
            if nbytes % per_in:
                raise ValueError("an array of whole pixels is needed")
            count = nbytes // per_in
            o = given[i] if given is not None else self.torch.empty(count * per_out, dtype=self.torch.uint8, device=self.tdev)
            if o.numel() * o.element_size() < count * per_out:
                raise ValueError("an output of at least the converted size is needed")
            outs.append(o)
            descs[i] = HsvaDesc(self._ptr(t), self._ptr(o), count, op)
        res = (Result * max(n, 1))()
        _check(self.lib, self.lib.spng_hsva_batch(self.ctx, descs, n, None, res))
        return outs, list(res)[:n]

    def hsva(self, pixels: bytes, op):
        """[PNG.RGBA<UInt8>].map(HSVA.init(r:g:b:a:)) (HSVA_FROM_RGBA8), [HSVA].map(\\.rgba) (HSVA_TO_RGBA8) or the (v, a) pairs of
        [HSVA] (HSVA_TO_VA8) as bytes (host order): -> (bytes, trapped pixels)"""
        if op not in _HSVA_BYTES:
            raise ValueError("op must be HSVA_FROM_RGBA8, HSVA_TO_RGBA8 or HSVA_TO_VA8")
        per_in, per_out = _HSVA_BYTES[op]
        if len(pixels) % per_in:
            raise ValueError("whole pixels are needed")
        n = len(pixels) // per_in
        out = (ctypes.c_uint8 * max(n * per_out, 1))()
        res = Result()
        _check(self.lib, self.lib.spng_hsva(self.ctx, _cbuf(pixels), n, int(op), out, ctypes.byref(res)))
        return bytes(out[:n * per_out]), int(res.aux[0])

    def luminance_batch(self, arrays, ops, outs=None):
        """spng_luminance_batch on device tensors: every tensor of `arrays` holds whole RGBA<UInt8> pixels and is reduced into the
        tensor of `outs` at its place (never in place: the element sizes differ), or into a new uint8 tensor where outs is None --
        one byte a pixel for LUMINANCE_V8, (l, a) for LUMINANCE_VA8.  ops: one value, or one per array.  -> (list of output
        tensors, list[Result])"""
        n = len(arrays)
        descs = (LuminanceDesc * max(n, 1))()
        given, outs = outs, []
        for i, t in enumerate(arrays):
            op = pick(ops, i)
            if op not in (LUMINANCE_V8, LUMINANCE_VA8):
                raise ValueError("op must be LUMINANCE_V8 or LUMINANCE_VA8")
            nbytes = t.numel() * t.element_size()
            if nbytes % 4:
                raise ValueError("an array of whole pixels is needed")
            count = nbytes // 4
            o = given[i] if given is not None else self.torch.empty(count * op, dtype=self.torch.uint8, device=self.tdev)
            if o.numel() * o.element_size() < count * op:
                raise ValueError("an output of at least the converted size is needed")
            outs.append(o)
            descs[i] = LuminanceDesc(self._ptr(t), self._ptr(o), count, op)
        res = (Result * max(n, 1))()
        _check(self.lib, self.lib.spng_luminance_batch(self.ctx, descs, n, None, res))
        return outs, list(res)[:n]

    def luminance(self, pixels: bytes, op=LUMINANCE_V8) -> bytes:
        """[PNG.RGBA<UInt8>].map(COMPUTE_LUMINANCE) (Snippets/PNG/BasicEncoding.swift:63-71) as bytes: one a pixel for LUMINANCE_V8,
        (l, a) for LUMINANCE_VA8"""
        if op not in (LUMINANCE_V8, LUMINANCE_VA8):
            raise ValueError("op must be LUMINANCE_V8 or LUMINANCE_VA8")
        if len(pixels) % 4:
            raise ValueError("whole pixels are needed")
        n = len(pixels) // 4
        out = (ctypes.c_uint8 * max(n * op, 1))()
        res = Result()
        _check(self.lib, self.lib.spng_luminance(self.ctx, _cbuf(pixels), n, int(op), out, ctypes.byref(res)))
        return bytes(out[:n * op])

    def deflate(self, data: bytes, level: int, fmt=FORMAT_ZLIB, exponent: int = 15) -> bytes:
        """Whole-stream LZ77.Deflator (push(all, last: true) + concatenated pull()): -> stream bytes"""
        cap = self.lib.spng_deflate_bound(len(data))
        dst = (ctypes.c_uint8 * cap)()
        res = Result()
        _check(self.lib, self.lib.spng_deflate_window(self.ctx, _cbuf(data), len(data), fmt, level, exponent, dst, cap,
                                                      ctypes.byref(res)))
        if res.status != DONE:
            raise SpngError(res.status)
        return bytes(dst[:res.written])

    def deflate_resume(self, src, src_len, dst, level, state, last, fmt=FORMAT_ZLIB, exponent=15, hstate=(0, 0)):
        """One push of a stream that is compressed as it arrives (spng_deflate_resume_batch): src holds ALL input so far, dst the
        stream so far, state: a zero-initialised device tensor of spng_deflate_state_bytes() bytes kept between the calls, hstate
        what the previous call returned.  -> (Result, next hstate)"""
        desc = (StreamDesc * 1)(StreamDesc(self._ptr(src), int(src_len), self._ptr(dst), dst.numel(), fmt, exponent))
        lv = (ctypes.c_int32 * 1)(level)
        st = (ctypes.c_void_p * 1)(state.data_ptr())
        la = (ctypes.c_uint8 * 1)(1 if last else 0)
        hs = (ctypes.c_uint64 * 2)(int(hstate[0]), int(hstate[1]))
        res = (Result * 1)()
        _check(self.lib, self.lib.spng_deflate_resume_batch(self.ctx, desc, lv, st, la, hs, 1, None, res))
        r = res[0]
        return r, (r.aux[0], r.aux[1])

    def deflate_batch(self, streams, level, fmt=FORMAT_ZLIB, levels=None, exponents=None):
        """streams: list of uint8 device tensors -> (list of output tensors, list[Result]).  level / fmt: one value, or one per
        stream; levels: a level per stream (instead of `level`); exponents: a window exponent 8 ... 15 per stream (None or 0: 15,
        what PNG uses; spng_stream_desc.reserved)"""
        n = len(streams)
        caps = [self.lib.spng_deflate_bound(t.numel()) for t in streams]
        outs = [self.empty(c) for c in caps]
        descs = (StreamDesc * n)()
        for i, (t, o, c) in enumerate(zip(streams, outs, caps)):
            descs[i] = StreamDesc(self._ptr(t), t.numel(), self._ptr(o), int(c), pick(fmt, i), int(exponents[i]) if exponents is not None else 0)
        levels = (ctypes.c_int32 * n)(*[int(pick(level if levels is None else list(levels), i)) for i in range(n)])
        res = (Result * n)()
        _check(self.lib, self.lib.spng_deflate_batch(self.ctx, descs, levels, n, None, res))
        return outs, list(res)

    def adler32(self, data: bytes) -> int:
        out = ctypes.c_uint32(0)
        _check(self.lib, self.lib.spng_adler32(self.ctx, _cbuf(data), len(data), ctypes.byref(out)))
        return out.value


from .mirror import LZ77, PNG, Gzip  # noqa: E402,F401
