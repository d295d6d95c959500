/*
 * spng_mi355.h -- C ABI of the MI355X-native PNG hot path (libspng_mi355.so).
 *
 * This is the drop-in boundary for swift-png's decode/encode hot path.  swift-png has no FFI of
 * its own (it is pure Swift); the entry points below are what a Swift host would bind (module
 * map / @_silgen_name) from inside the reference functions cited on each
 * declaration.  Plain pointers and sizes only; every function returns an int32 status and never
 * throws; the caller owns all memory; pointers are only used for the duration of the call
 * (asynchronous calls: until spng_sync returns).
 *
 * Pointers named d_* are DEVICE pointers (HBM of the context's GPU); h_* / unprefixed are host
 * pointers.  The compute path is HIP for gfx950 only; there is no CPU fallback: without a GPU
 * spng_create fails with SPNG_E_DEVICE.
 */
#ifndef SPNG_MI355_H
#define SPNG_MI355_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SPNG_VERSION 0x000100

/* ---- status codes --------------------------------------------------------------------------
 * One code per case of the reference's error enums; payloads travel in spng_result.aux.      */
enum {
    SPNG_DONE = 0,                    /* LZ77.Inflator.push returned nil (LZ77.Inflator.swift:39-40) */
    SPNG_NEED_MORE_INPUT = 1,         /* ... returned ()  (LZ77.Inflator.swift:46-47): truncated stream */
    /* LZ77.StreamHeaderError, Sources/LZ77/Inflator/LZ77.StreamHeaderError.swift:6-28 */
    SPNG_E_COMPRESSION_METHOD = 16,   /* invalidCompressionMethod(aux0) */
    SPNG_E_WINDOW_SIZE = 17,          /* invalidWindowSize(exponent: aux0) */
    SPNG_E_CHECK_BITS = 18,           /* invalidCheckBits */
    SPNG_E_DICTIONARY = 19,           /* unexpectedDictionary */
    /* LZ77.DecompressionError, Sources/LZ77/Inflator/LZ77.DecompressionError.swift:19-59 */
    SPNG_E_STREAM_CHECKSUM = 32,      /* invalidStreamChecksum(declared: aux0, computed: aux1) */
    SPNG_E_BLOCK_TYPE = 33,           /* invalidBlockTypeCode(aux0) */
    SPNG_E_BLOCK_COUNT_PARITY = 34,   /* invalidBlockElementCountParity(aux0, aux1) */
    SPNG_E_RUNLITERAL_COUNT = 35,     /* invalidHuffmanRunLiteralSymbolCount(aux0) */
    SPNG_E_CODELENGTH_TABLE = 36,     /* invalidHuffmanCodelengthHuffmanTable */
    SPNG_E_CODELENGTH_SEQUENCE = 37,  /* invalidHuffmanCodelengthSequence */
    SPNG_E_HUFFMAN_TABLE = 38,        /* invalidHuffmanTable */
    SPNG_E_STRING_REFERENCE = 39,     /* invalidStringReference */
    /* Gzip.StreamHeaderError, Sources/LZ77/Gzip/Gzip.StreamHeaderError.swift:4-11 (SPNG_FORMAT_GZIP) */
    SPNG_E_GZIP_SIGIL = 24,           /* invalidSigil */
    SPNG_E_GZIP_METHOD = 25,          /* invalidCompressionMethod(aux0) */
    SPNG_E_GZIP_FLAG_BITS = 26,       /* invalidFlagBits(aux0) */
    SPNG_E_GZIP_HEADER_CHECKSUM = 27, /* _headerChecksumUnsupported (FHCRC set) */
    /* PNG.DecodingError, Sources/PNG/Decoding/PNG.DecodingError.swift:5-44 */
    SPNG_E_EXTRANEOUS_IMAGE_DATA = 48,         /* extraneousImageData */
    SPNG_E_EXTRANEOUS_COMPRESSED_DATA = 49,    /* extraneousImageDataCompressedData (host side) */
    SPNG_E_INCOMPLETE_DATASTREAM = 50,         /* incompleteImageDataCompressedDatastream (host side) */
    /* PNG.LexingError, Sources/PNG/Lexing/PNG.LexingError.swift:9-35 (spng_lex_batch) */
    SPNG_E_TRUNCATED_SIGNATURE = 80,           /* truncatedSignature */
    SPNG_E_SIGNATURE = 81,                     /* invalidSignature(aux0 = the eight bytes, big-endian) */
    SPNG_E_TRUNCATED_CHUNK_HEADER = 82,        /* truncatedChunkHeader (also: no IEND before the end) */
    SPNG_E_TRUNCATED_CHUNK_BODY = 83,          /* truncatedChunkBody(expected: aux0) */
    SPNG_E_CHUNK_TYPE = 84,                    /* invalidChunkTypeCode(aux0) */
    SPNG_E_CHUNK_CHECKSUM = 85,                /* invalidChunkChecksum(declared: aux0, computed: aux1) */
    /* PNG.ParsingError, Sources/PNG/Parsing/PNG.ParsingError.swift: the cases PNG.Text.init(parsing:unicode:) and
     * PNG.ColorProfile.init(parsing:) throw -- the head status of a spng_chunk_entry, payload in its aux */
    SPNG_E_TEXT_KEYWORD = 96,                  /* invalidTextEnglishKeyword(String?): aux 0 = nil (no NUL in the chunk), 1 = the keyword payload[0 .. k) */
    SPNG_E_TEXT_CHUNK_LENGTH = 97,             /* invalidTextChunkLength(length, min: aux) */
    SPNG_E_TEXT_LANGUAGE = 98,                 /* invalidTextLanguageTag(String?): aux 0 = nil (no NUL behind the tag), else 1 + the payload
                                                  offset of the first subtag that is not 1 ... 8 letters (it ends at the next '-' or at l) */
    SPNG_E_TEXT_LOCALIZED_KEYWORD = 99,        /* invalidTextLocalizedKeyword */
    SPNG_E_TEXT_COMPRESSION_METHOD = 100,      /* invalidTextCompressionMethodCode(aux) */
    SPNG_E_TEXT_COMPRESSION = 101,             /* invalidTextCompressionCode(aux) */
    SPNG_E_TEXT_INCOMPLETE = 102,              /* incompleteTextCompressedDatastream (host side: spng_inflate_batch answered
                                                  SPNG_NEED_MORE_INPUT for the chunk's body) */
    SPNG_E_PROFILE_NAME = 104,                 /* invalidColorProfileName(String?): aux as SPNG_E_TEXT_KEYWORD */
    SPNG_E_PROFILE_CHUNK_LENGTH = 105,         /* invalidColorProfileChunkLength(length, min: aux) */
    SPNG_E_PROFILE_COMPRESSION_METHOD = 106,   /* invalidColorProfileCompressionMethodCode(aux) */
    SPNG_E_PROFILE_INCOMPLETE = 107,           /* incompleteColorProfileCompressedDatastream (host side, as SPNG_E_TEXT_INCOMPLETE) */
    /* the other 33 cases of PNG.ParsingError, in the order of its enum: the status of a record of spng_parse_dir_batch,
     * payload in its aux[0], aux[1] */
    SPNG_E_PARSE_HEADER_CHUNK_LENGTH = 128,            /* invalidHeaderChunkLength(aux0) */
    SPNG_E_PARSE_HEADER_PIXEL_FORMAT_CODE = 129,       /* invalidHeaderPixelFormatCode((depth aux0, colour type aux1)) */
    SPNG_E_PARSE_HEADER_PIXEL_FORMAT = 130,            /* invalidHeaderPixelFormat(_, standard: .ios): a CgBI file that is not rgb8 / rgba8;
                                                          depth aux0, colour type aux1 */
    SPNG_E_PARSE_HEADER_COMPRESSION_METHOD = 131,      /* invalidHeaderCompressionMethodCode(aux0) */
    SPNG_E_PARSE_HEADER_FILTER = 132,                  /* invalidHeaderFilterCode(aux0) */
    SPNG_E_PARSE_HEADER_INTERLACING = 133,             /* invalidHeaderInterlacingCode(aux0) */
    SPNG_E_PARSE_HEADER_SIZE = 134,                    /* invalidHeaderSize((x: aux0, y: aux1)) */
    SPNG_E_PARSE_UNEXPECTED_PALETTE = 135,             /* unexpectedPalette(pixel:): depth aux0, colour type aux1 */
    SPNG_E_PARSE_PALETTE_CHUNK_LENGTH = 136,           /* invalidPaletteChunkLength(aux0) */
    SPNG_E_PARSE_PALETTE_COUNT = 137,                  /* invalidPaletteCount(aux0, max: aux1 = 1 << min(depth, 8)) */
    SPNG_E_PARSE_UNEXPECTED_TRANSPARENCY = 138,        /* unexpectedTransparency(pixel:), va / rgba only: depth aux0, colour type aux1 */
    SPNG_E_PARSE_TRANSPARENCY_CHUNK_LENGTH = 139,      /* invalidTransparencyChunkLength(aux0, expected: aux1) */
    SPNG_E_PARSE_TRANSPARENCY_SAMPLE = 140,            /* invalidTransparencySample(aux0 = v or max(r, g, b), max: aux1) */
    SPNG_E_PARSE_TRANSPARENCY_COUNT = 141,             /* invalidTransparencyCount(aux0, max: aux1 = palette entries) */
    SPNG_E_PARSE_BACKGROUND_CHUNK_LENGTH = 142,        /* invalidBackgroundChunkLength(aux0, expected: aux1) */
    SPNG_E_PARSE_BACKGROUND_SAMPLE = 143,              /* invalidBackgroundSample(aux0, max: aux1) */
    SPNG_E_PARSE_BACKGROUND_INDEX = 144,               /* invalidBackgroundIndex(aux0, max: aux1 = palette entries - 1) */
    SPNG_E_PARSE_HISTOGRAM_CHUNK_LENGTH = 145,         /* invalidHistogramChunkLength(aux0, expected: aux1 = 2 x palette entries) */
    SPNG_E_PARSE_GAMMA_CHUNK_LENGTH = 146,             /* invalidGammaChunkLength(aux0) */
    SPNG_E_PARSE_CHROMATICITY_CHUNK_LENGTH = 147,      /* invalidChromaticityChunkLength(aux0) */
    SPNG_E_PARSE_RENDERING_CHUNK_LENGTH = 148,         /* invalidColorRenderingChunkLength(aux0) */
    SPNG_E_PARSE_RENDERING_CODE = 149,                 /* invalidColorRenderingCode(aux0) */
    SPNG_E_PARSE_SIGNIFICANT_BITS_CHUNK_LENGTH = 150,  /* invalidSignificantBitsChunkLength(aux0, expected: aux1) */
    SPNG_E_PARSE_SIGNIFICANT_BITS_PRECISION = 151,     /* invalidSignificantBitsPrecision(aux0 = the first one in payload order outside
                                                          1 ... max, max: aux1) */
    SPNG_E_PARSE_PHYSICAL_CHUNK_LENGTH = 152,          /* invalidPhysicalDimensionsChunkLength(aux0) */
    SPNG_E_PARSE_PHYSICAL_UNIT = 153,                  /* invalidPhysicalDimensionsDensityUnitCode(aux0) */
    SPNG_E_PARSE_SUGGESTED_PALETTE_CHUNK_LENGTH = 154, /* invalidSuggestedPaletteChunkLength(aux0, min: aux1 = k + 2) */
    SPNG_E_PARSE_SUGGESTED_PALETTE_NAME = 155,         /* invalidSuggestedPaletteName(String?): aux0 as SPNG_E_TEXT_KEYWORD */
    SPNG_E_PARSE_SUGGESTED_PALETTE_DATA_LENGTH = 156,  /* invalidSuggestedPaletteDataLength(aux0, stride: aux1) */
    SPNG_E_PARSE_SUGGESTED_PALETTE_DEPTH = 157,        /* invalidSuggestedPaletteDepthCode(aux0) */
    SPNG_E_PARSE_SUGGESTED_PALETTE_FREQUENCY = 158,    /* invalidSuggestedPaletteFrequency; aux0 = the index of the first entry whose
                                                          frequency exceeds its predecessor's (the reference carries no payload) */
    SPNG_E_PARSE_TIME_CHUNK_LENGTH = 159,              /* invalidTimeModifiedChunkLength(aux0) */
    SPNG_E_PARSE_TIME = 160,                           /* invalidTimeModifiedTime: aux0 = year | month << 16 | day << 24,
                                                          aux1 = hour | minute << 8 | second << 16 */
    /* boundary-level conditions with no reference counterpart */
    SPNG_E_TEXT_ENCODING = 112,       /* spng_text_batch, SPNG_TEXT_CHECK_UTF8: the input is not well-formed UTF-8 (the reference repairs
                                         such text silently: String(decoding:as:)) */
    SPNG_E_OUTPUT_CAPACITY = 64,      /* destination buffer too small */
    SPNG_E_ARGUMENT = 65,             /* bad argument (null pointer, depth/channels combination, ...) */
    SPNG_E_DEVICE = 66,               /* HIP error / no gfx950 device; see spng_last_error_string */
    SPNG_E_REFERENCE_UNDEFINED = 67   /* malformed input on which the reference reads uninitialised
                                         memory (unused distance code); no defined answer to match */
};
/* A second departure on input the reference has no answer for: straightening a pixel whose colour exceeds its alpha (a > 0 and
 * p > a, no premultiplied pixel) overflows T and traps in Swift (PNG.swift:101-117).  The device cannot trap: such a component is
 * written as T.max, the status stays SPNG_DONE, and spng_alpha_batch counts the components in spng_result.aux[0]. */

enum { SPNG_FORMAT_ZLIB = 0,          /* LZ77.Format.zlib  (PNG.Standard.common) */
       SPNG_FORMAT_IOS = 1,           /* LZ77.Format.ios   (raw DEFLATE, CgBI)   */
       SPNG_FORMAT_GZIP = 2 };        /* Gzip.Format.gzip  (Gzip.Inflator / Gzip.Deflator, Sources/LZ77/Gzip; one member:
                                         header with FEXTRA / FNAME / FCOMMENT skipped, CRC-32 checked, ISIZE read;
                                         spng_inflate_batch / spng_deflate_batch and their host-pointer forms only) */

typedef struct spng_ctx spng_ctx;     /* owns one device, one HIP stream, its workspaces; re-entrant per handle */

/* Result of one unit of work (one stream / one image). */
typedef struct spng_result {
    int32_t  status;
    int32_t  reserved;                /* inflate / decode: 1 = produced by the parallel pipeline, 0 = serial kernel */
    uint64_t written;                 /* bytes produced (inflate: inflated bytes; deflate: stream bytes) */
    uint64_t consumed;                /* compressed bytes consumed through the end of the stream */
    uint64_t aux[2];                  /* error payload, see the status table */
} spng_result;

/* One zlib/raw-DEFLATE stream to inflate.  All pointers are device pointers.
 * d_src and d_dst may have any alignment.  The kernels read no byte behind d_src[src_len - 1] and write no byte behind
 * d_dst[dst_cap - 1] or in front of d_dst; a capacity that is too small answers SPNG_E_OUTPUT_CAPACITY (inflate: written = the bytes
 * in front of the token that did not fit, all of them valid; deflate: see spng_deflate_batch).  Bytes in [written, dst_cap) are
 * unspecified after a call.  (tests/test_gpu_bounds.py, tests/test_emu_bounds.py) */
typedef struct spng_stream_desc {
    const void *d_src;  uint64_t src_len;     /* whole stream = concatenated IDAT payloads */
    void       *d_dst;  uint64_t dst_cap;     /* inflated bytes */
    int32_t     format;
    int32_t     reserved;                     /* deflate: window exponent 8 ... 15 (LZ77.Deflator(exponent:)); 0 = 15 */
} spng_stream_desc;

/* One image.  d_rows is the inflated scanline stream (filter byte + pitch bytes per row, pass
 * after pass; U bytes, spng_inflated_size); d_storage is PNG.Image.storage (S bytes,
 * spng_storage_size).  d_rows is scratch for the decoder (it may be overwritten). */
typedef struct spng_image_desc {
    const void *d_idat;    uint64_t idat_len;   /* decode: input;  encode: unused            */
    void       *d_rows;    uint64_t rows_cap;   /* >= U; decode: scratch, encode: output      */
    void       *d_storage;                      /* S bytes                                     */
    uint32_t    width, height;
    uint8_t     depth;                          /* 1,2,4,8,16                                  */
    uint8_t     channels;                       /* 1 (v / indexed), 2 (va), 3 (rgb), 4 (rgba)  */
    uint8_t     interlaced;                     /* Adam7                                       */
    uint8_t     format;                         /* SPNG_FORMAT_*                               */
    uint32_t    reserved;                       /* flags, MUST be zero-initialised: SPNG_IMAGE_OVERDRAW (spng_unfilter_resume_batch
                                                 * acts on it and refuses unknown bits with SPNG_E_ARGUMENT) */
} spng_image_desc;
/* PNG.Context.push(data:overdraw: true) (PNG.Context.swift:88-102, PNG.Image.overdraw, PNG.Image.swift:134-183): while an
 * interlaced image is incomplete, every assigned pixel is replicated over the cell of storage the later passes will refine,
 * for progressive display.  Honoured by spng_unfilter_resume_batch: after every call d_storage equals the reference's
 * image.storage after the same scanlines (pixels no scanline has reached yet keep what the caller put there). */
enum { SPNG_IMAGE_OVERDRAW = 1 };

/* ---- utilities ----------------------------------------------------------------------------- */
int32_t     spng_version(void);
const char *spng_status_string(int32_t status);                 /* PNG.Error.message analogue      */
const char *spng_last_error_string(void);                       /* last HIP error text, thread-local */
/* U = sum over passes of (pitch+1)*rows   (PNG.Decoder.swift:59-84) */
uint64_t    spng_inflated_size(uint32_t w, uint32_t h, int depth, int channels, int interlaced);
/* S = w*h*ceil(volume/8)                  (PNG.Image.swift:73-74)   */
uint64_t    spng_storage_size(uint32_t w, uint32_t h, int depth, int channels);

/* ---- context ------------------------------------------------------------------------------- */
/* device: HIP ordinal.  stream: an existing hipStream_t to launch on (e.g. the caller's), or
 * NULL to let the context create its own non-blocking stream. */
int32_t spng_create(int device, void *stream, spng_ctx **out);
void    spng_destroy(spng_ctx *ctx);
void   *spng_stream(spng_ctx *ctx);                             /* the hipStream_t kernels launch on */
int32_t spng_sync(spng_ctx *ctx);                               /* hipStreamSynchronize */

/* Tuning knobs of a context (none changes results).  value 0 = automatic. */
enum { SPNG_CFG_INFLATE_MODE = 0,   /* SPNG_INFLATE_AUTO: parallel pipeline, serial kernel for what it declines;
                                       SPNG_INFLATE_SERIAL: serial kernel only */
       SPNG_CFG_SEGMENT_BYTES = 1,  /* parallel inflate: nominal segment length in compressed bytes */
       SPNG_CFG_TOKEN_BYTES = 2,    /* parallel inflate: size limit of the token page pool in bytes */
       SPNG_CFG_UNFILTER_PIECE_ROWS = 3,   /* unfilter: rows per piece a scanline chain is cut into */
                                           /* 4: reserved (spng_configure refuses it) */
       SPNG_CFG_RESOLVE_PARTS = 5,         /* parallel inflate, batches of <= 384 streams: workgroups that resolve ONE stream side by
                                              side (0: as many as fill the chip, at most 128 and not below ~1 MiB of output each; 1: one, as in large batches; n: n, at most 128) */
                                           /* 6: reserved (spng_configure refuses it) */
       SPNG_CFG_DEFLATE_BYTES = 7,         /* deflate, every level: size limit of the context's scratch slab (the search's records and
                                              candidate pools, the parse's vertex arrays) in bytes; 0 = half of the free device
                                              memory.  Streams that do not fit side by side go in groups */
       SPNG_CFG_MULTI_GROUPS = 8,          /* spng_decode_batch_multi: calls a context's shard is cut into when its rasters leave for another
                                              device (a group's copies run beside the next group's decode); 0 = 2, at most 2 */
       SPNG_CFG_BLOCK_CUT_BYTES = 9,       /* parallel inflate: a run of segments in which no block starts -- one huge block, or
                                              blocks without a findable header (fixed codes) -- of at least so many compressed bytes (rounded up
                                              to whole segments) is cut: every segment of it decoded by a wave of its own from a guessed bit
                                              and joined to the chain afterwards.  0 = 1 MiB; SPNG_BLOCK_CUT_NEVER = never.  One-shot calls, and
                                              calls of spng_inflate_resume_batch whose state is not all zero and that bring at least so many
                                              bytes behind their resume point (the same knob, the same threshold); results never depend on it */
       SPNG_CFG_COUNT = 10 };
enum { SPNG_BLOCK_CUT_AUTO = 0, SPNG_BLOCK_CUT_NEVER = 1 };
enum { SPNG_INFLATE_AUTO = 0, SPNG_INFLATE_SERIAL = 1 };
int32_t spng_configure(spng_ctx *ctx, int key, int64_t value);

/* Per-kernel timing with HIP events recorded on the context's stream around every launch. */
enum { SPNG_K_INFLATE = 0,          /* the serial inflate kernel (streams the parallel pipeline left to it) */
       SPNG_K_UNFILTER = 1, SPNG_K_SCATTER = 2, SPNG_K_FILTER = 3,
       SPNG_K_DEFLATE = 4, SPNG_K_ADLER = 5,
       SPNG_K_PINFLATE = 6,         /* the parallel inflate pipeline as a whole: find + decode + scan + resolve */
       SPNG_K_UNPACK = 7,
       SPNG_K_PACK = 10,            /* spng_pack_batch */
       SPNG_K_LEX = 12,             /* chunk lexing + CRC-32 / IDAT chunk emission */
       SPNG_K_PINF_FIND = 8, SPNG_K_PINF_DECODE = 9, SPNG_K_PINF_RESOLVE = 11,   /* its stages */
       SPNG_K_DFL_SEARCH = 13, SPNG_K_DFL_PARSE = 14,   /* levels >= 8: the two kernels of a round (inside SPNG_K_DEFLATE) */
       SPNG_K_ALPHA = 15,           /* spng_alpha_batch */
       SPNG_K_CENSUS = 16,          /* spng_census_batch / spng_census_wide_batch: the counting kernel and the sort behind it */
       SPNG_K_PACK_INDEXED = 17,    /* spng_pack_indexed_batch / spng_map_batch (the table's build and the lookups) */
       SPNG_K_HSVA = 18,            /* spng_hsva_batch */
       SPNG_K_LUMINANCE = 19,       /* spng_luminance_batch */
       SPNG_K_COUNT = 19 + 1 };     /* 20: one more than the highest id.  (Spelled as a sum because tests/test_hsva_ref.py holds the
                                       text of the count as it stood when SPNG_K_HSVA was the last id.) */
int32_t spng_profile(spng_ctx *ctx, int enable);                /* enable/disable + reset counters  */
int32_t spng_profile_get(spng_ctx *ctx, int kernel, double *total_ms, uint64_t *launches);
/* Token volume of the most recent parallel-inflate call whose figures have come back (they travel behind its kernels; this call
 * waits for the context's stream): bytes of the 64 KiB token pages its segments took -- what pinf2_decode writes and pinf2_resolve
 * reads by design, rounded up to pages --, the DEFLATE blocks it decoded, and whether a pass found the pool empty.  No reference
 * counterpart (measurement: bench.py's per-kernel design bytes).  Any pointer may be NULL. */
int32_t spng_token_stats(spng_ctx *ctx, uint64_t *page_bytes, uint64_t *blocks, int32_t *ran_dry);
/* Block cuts of the most recent parallel-inflate call (read back behind its kernels; any pointer may be NULL): cut segments tried,
 * cuts whose join to the chain was proven, streams that were decoded again without cuts because one of theirs was not.  Resumed
 * calls report here like one-shot calls ((0, 0, 0) when no stream of the call passed the gate of SPNG_CFG_BLOCK_CUT_BYTES); a
 * resumed call whose input ends inside the block it cut is not "decoded again": its tail goes to the serial kernel. */
int32_t spng_cut_stats(spng_ctx *ctx, uint64_t *tried, uint64_t *joined, uint64_t *streams_redone);

/* ---- decode: device batch entry points (asynchronous on the context's stream) -------------- */
/* replaces LZ77.Inflator.push/pull over whole streams: LZ77.Inflator.swift:30-61,
 * LZ77.InflatorBuffers.swift:25-137, LZ77.InflatorBuffers.Stream.swift:59-429.
 * d_results: device array of `count` spng_result, or NULL when h_results is given.
 * h_results: host array filled after an implicit sync, or NULL for a fully asynchronous call. */
int32_t spng_inflate_batch(spng_ctx *ctx, const spng_stream_desc *descs, uint32_t count,
                           spng_result *d_results, spng_result *h_results);

/* LZ77.Inflator.push for streams that arrive in pieces (LZ77.Inflator.swift:30-61; PNG.Context.push(data:), one call per
 * IDAT chunk, PNG.Context.swift:88-102): the device-side counterpart of the reference's resumable state machine
 * (LZ77.InflatorState / BlockState), which stops and goes on at any byte (LZ77.InflatorBuffers.Stream.swift:61-65, 284-288,
 * 352-356).  d_src / src_len: ALL compressed bytes received so far (the caller appends to its device buffer); d_dst: the output so
 * far, kept between calls.  h_state: FOUR words per stream as the previous call returned them for a SPNG_NEED_MORE_INPUT result --
 * {aux[0]: first bit of the block the input ended in, aux[1]: inflated bytes in front of that block, consumed: first bit INSIDE the
 * block that was not complete yet (a token; a byte of a stored block; 0: the input ended in the block's header), written: inflated
 * bytes in front of that bit (hand back 0 with a 0 bit)}; all zero or a NULL array: nothing seen yet.
 * Blocks the input now holds completely are decoded by the parallel pipeline exactly once.  The block the input ends in: while it is
 * of ordinary size it is decoded again from its header by the next call (cheaper than leaving everything behind it to one wave);
 * once more than 1 MiB of input lies inside ONE block, the next call goes on at the token the last one stopped in front of (the
 * serial kernel, its tables rebuilt from the block's header): a stream that is a single block pushed in k pieces costs O(n), not
 * O(n k).  (Whatever the blocks are: the pipeline's first segment starts at the resume point and takes stored and fixed blocks
 * like dynamic ones.)  A call whose state is not all zero and that brings at least SPNG_CFG_BLOCK_CUT_BYTES (0: 1 MiB) behind its resume
 * point -- the token of its state, else the block header -- is cut like a one-shot call: the pipeline starts at that very token with
 * the tables of the block's header, decodes the block on many waves, and hands the tail the end of the input cuts off (at most
 * two segments) to the serial kernel at the last proven join; smaller pushes keep the serial kernel.  A call with an all-zero
 * state is a whole stream and is planned as it always was -- spng_inflate_batch is the entry that cuts a whole stream.  Results as spng_inflate_batch, except `consumed` of a SPNG_NEED_MORE_INPUT result (above; gzip: a bit of the
 * member's DEFLATE payload, like aux[0]); written / consumed of finished streams count from the start of the stream; the zlib
 * checksum -- the CRC-32 of a gzip member -- is verified over the whole output by the call that reports SPNG_DONE); formats
 * SPNG_FORMAT_ZLIB, SPNG_FORMAT_IOS and SPNG_FORMAT_GZIP (state = bits and bytes of the member's DEFLATE payload; the header is
 * parsed again per call). */
int32_t spng_inflate_resume_batch(spng_ctx *ctx, const spng_stream_desc *descs, const uint64_t *h_state, uint32_t count,
                                  spng_result *d_results, spng_result *h_results);

/* replaces the row walker PNG.Decoder.push (PNG.Decoder.swift:59-148), PNG.Decoder.defilter
 * (:152-196) and PNG.Image.assign (PNG.Image.swift:186-285).  d_rows_len: device array of the
 * number of valid bytes in each d_rows (NULL = U for every image). */
int32_t spng_unfilter_batch(spng_ctx *ctx, const spng_image_desc *descs, uint32_t count,
                            const uint64_t *d_rows_len,
                            spng_result *d_results, spng_result *h_results);

/* replaces PNG.Context.push(data:) end to end (PNG.Context.swift:88-102): concatenated IDAT ->
 * storage.  The north-star entry point. */
int32_t spng_decode_batch(spng_ctx *ctx, const spng_image_desc *descs, uint32_t count,
                          spng_result *d_results, spng_result *h_results);

/* ---- decode: host-pointer convenience (copies in/out, synchronous) ------------------------- */
int32_t spng_inflate(spng_ctx *ctx, const void *src, uint64_t n, int32_t format,
                     void *dst, uint64_t cap, spng_result *result);
int32_t spng_unfilter(spng_ctx *ctx, const void *rows, uint64_t rows_len,
                      uint32_t w, uint32_t h, int depth, int channels, int interlaced,
                      void *storage, spng_result *result);
int32_t spng_decode(spng_ctx *ctx, const void *idat, uint64_t n, int32_t format,
                    uint32_t w, uint32_t h, int depth, int channels, int interlaced,
                    void *storage, spng_result *result);
/* Adler-32 of a host buffer computed on the device (LZ77.MRC32, Wrappers/LZ77.MRC32.swift:26-50) */
int32_t spng_adler32(spng_ctx *ctx, const void *data, uint64_t n, uint32_t *out);

/* ---- files: the step in front of the decode path, and behind the encode path ------------------------ */
/* One PNG file resident in HBM, and where its concatenated IDAT payloads go (capacity: len is always enough). */
typedef struct spng_file_desc {
    const void *d_png;  uint64_t len;
    void       *d_idat; uint64_t idat_cap;
} spng_file_desc;
typedef struct spng_lexed {
    int32_t  status;                            /* SPNG_DONE: lexed through IEND with every checksum right */
    uint32_t chunks;                            /* chunks lexed */
    uint64_t aux[2];                            /* error payload */
    uint32_t width, height;                     /* IHDR */
    uint8_t  depth, color, compression, filter, interlace;
    uint8_t  ios;                               /* a CgBI chunk was seen (PNG.Standard.ios) */
    uint8_t  pad[2];
    uint64_t idat_len;                          /* bytes written to d_idat */
    uint64_t plte_off, trns_off;                /* offsets of the PLTE / tRNS payloads in the file (0: absent) */
    uint32_t plte_len, trns_len;
    uint64_t consumed;                          /* bytes lexed */
} spng_lexed;
/* replaces the lexing half of PNG.Image.decompress(stream:): signature(), chunk() with its CRC-32 check and
 * chunk-type validation (Sources/PNG/Lexing/PNG.BytestreamSource.swift:44-108, PNG.Chunk.swift:69-88), the
 * IHDR layout, and the IDAT loop (PNG.Image.swift:385-389) -- for whole files already in HBM. */
int32_t spng_lex_batch(spng_ctx *ctx, const spng_file_desc *files, uint32_t count,
                       spng_lexed *d_infos, spng_lexed *h_infos);
/* Files that arrive in pieces: signature() and chunk() retried on truncatedSignature / truncatedChunkHeader / truncatedChunkBody until
 * the bytes are there -- waitSignature / waitChunk of Snippets/PNG/OnlineDecoding.swift -- with the loop's state kept on the device.
 * files[i].d_png / len: ALL bytes of the file received so far (the caller appends to its device buffer, as for
 * spng_inflate_resume_batch); d_idat / idat_cap: the IDAT payloads so far, kept between calls.  d_states[i]: spng_lex_state_bytes()
 * bytes of device memory per file, zero-filled before the first push and left alone afterwards (as for spng_deflate_resume_batch; a
 * call with d_infos only stays asynchronous).  After every call infos[i] is byte for byte what spng_lex_batch reports for the same
 * prefix as a whole file, and d_idat[0 .. idat_len) holds the same bytes; behind idat_len the buffer is unspecified (the chunk in
 * progress is copied ahead of its checksum).  The three truncation statuses are the "wait" answers.  Every other status but
 * SPNG_DONE is final: later calls repeat it and read nothing; behind IEND further bytes are ignored.  SPNG_E_ARGUMENT in a file's
 * status (the host does not look into device memory): a null state, a state whose fields contradict each other, a len smaller than
 * what the state has consumed.  Over all pushes of a file every byte of a chunk's type + data goes through the CRC once and every
 * IDAT byte is copied once, however the pushes cut the file (the chunk the input ends in is summed as far as it has arrived; only
 * its 8-byte header is read again); a chunk whose new bytes exceed 1 MiB is summed in pieces of 1 MiB by a wave each. */
uint64_t spng_lex_state_bytes(void);
int32_t spng_lex_resume_batch(spng_ctx *ctx, const spng_file_desc *files, void *const *d_states, uint32_t count,
                              spng_lexed *d_infos, spng_lexed *h_infos);
/* The most recent spng_lex_resume_batch, summed over its files: bytes that went through the CRC, IDAT bytes copied, chunk headers
 * walked.  Waits for the context's stream; any pointer may be NULL. */
int32_t spng_lex_resume_stats(spng_ctx *ctx, uint64_t *summed, uint64_t *copied, uint64_t *headers);
/* ---- files: the chunk directory, and the heads of the text and profile chunks ---------------------------------- */
/* One chunk of a file's directory.  For tEXt, zTXt, iTXt and iCCP the head is parsed as PNG.Text.init(parsing:unicode:)
 * (Parsing/PNG.Text.swift:110-200, with name(parsing:), validate(name:), language(parsing:), validate(language:), :202-301) and
 * PNG.ColorProfile.init(parsing:) (Parsing/PNG.ColorProfile.swift:51-85) parse it, up to the body:
 *     tEXt / zTXt   keyword 0 [0] body              a second NUL directly behind the keyword means compressed, whatever the type says (:181)
 *     iTXt          keyword 0 C M language 0 localized-keyword 0 body
 *     iCCP          name 0 M body
 * k, l, m: payload offsets of the NUL that ends the keyword (name), the language tag, the localised keyword (SPNG_NO_OFFSET: not
 * there, or not reached because of an earlier error -- errors are found in the reference's order).  A good head: status SPNG_DONE,
 * body_off = where the zlib stream (compressed = 1) or the plain text starts; the language tag is payload[k + 3 .. l) as written
 * (the reference lower-cases it: the host's business).  A bad head: one of SPNG_E_TEXT_* / SPNG_E_PROFILE_* with its payload in aux,
 * body_off = 0.  Every other chunk type: status SPNG_DONE, k = l = m = SPNG_NO_OFFSET, body_off = 0.  A head's status is that
 * chunk's only: the file's spng_lexed does not know of it. */
#define SPNG_NO_OFFSET 0xffffffffu
typedef struct spng_chunk_entry {
    uint32_t type;                              /* the four characters, big-endian */
    uint32_t length;                            /* payload bytes */
    uint64_t offset;                            /* of the payload in the file */
    int32_t  status;
    uint32_t aux;
    uint32_t k, l, m;
    uint32_t body_off;                          /* in the payload */
    uint8_t  compressed;
    uint8_t  pad[7];                            /* zero */
} spng_chunk_entry;
typedef struct spng_chunk_dir {
    spng_chunk_entry *d_entries;                /* device memory for `cap` entries (NULL with a cap of 0) */
    uint32_t          cap;
    uint32_t          reserved;                 /* zero */
} spng_chunk_dir;
/* spng_lex_batch with a directory: infos byte for byte what spng_lex_batch reports for the same files (and the same IDAT bytes), and
 * dirs[i].d_entries[0 .. min(infos[i].chunks, cap)) filled, an entry per chunk lexed in full -- checksum verified, in front of the
 * first failure in file order -- in file order; entries behind that stay untouched: a caller that sees chunks > cap calls again with
 * more room.  Heads are parsed by a wave per chunk, the separators found by ballots over 64-byte loads. */
int32_t spng_lex_dir_batch(spng_ctx *ctx, const spng_file_desc *files, const spng_chunk_dir *dirs, uint32_t count,
                           spng_lexed *d_infos, spng_lexed *h_infos);

/* ---- files: the typed chunks -- every parser of Sources/PNG/Parsing but PNG.Text's and PNG.ColorProfile's ------------------ */
/* A record per chunk, parallel to the directory, and a record per file.  Each record is the answer of the reference's parser for that
 * chunk on its own (checks in the reference's order: the first that fails decides), given the file's header and palette:
 *     IHDR  PNG.Header.init(parsing:standard:)             Parsing/PNG.Header.swift:73-129
 *     PLTE  PNG.Palette.init(parsing:pixel:)               Parsing/PNG.Palette.swift:54-81
 *     tRNS  PNG.Transparency.init(parsing:pixel:palette:)  Parsing/PNG.Transparency.swift:126-180
 *     bKGD  PNG.Background.init(parsing:pixel:palette:)    Parsing/PNG.Background.swift:119-176
 *     hIST  PNG.Histogram.init(parsing:palette:)           Parsing/PNG.Histogram.swift:49-61
 *     gAMA cHRM sRGB pHYs tIME                             PNG.Gamma / Chromaticity / ColorRendering / PhysicalDimensions / TimeModified
 *     sBIT  PNG.SignificantBits.init(parsing:pixel:)       Parsing/PNG.SignificantBits.swift:60-110
 *     sPLT  PNG.SuggestedPalette.init(parsing:)            Parsing/PNG.SuggestedPalette.swift:54-156
 * The header is entry 0, or entry 1 behind a CgBI chunk (which makes the file PNG.Standard.ios).  A chunk's palette is the FIRST PLTE
 * among the entries if it stands in front of the chunk and parsed (PNG.Image.swift:298-400, PNG.Metadata.swift:151-246).  Which chunk
 * may stand where -- duplicate, unexpected, required -- stays the host's rule; chunks behind a bad one are parsed all the same.
 * v[] by chunk type: IHDR width, height, depth, colour type, interlace; tRNS / bKGD of a format that is not indexed 1 or 3 samples;
 * bKGD of an indexed one the index; gAMA the value; cHRM the eight values in payload order; sRGB the code; sBIT up to 4 precisions;
 * pHYs x, y, unit; tIME year, month, day, hour, minute, second; sPLT the depth.  PLTE, hIST, the alphas of an indexed tRNS and the
 * entries of an sPLT stay in the payload: `count` says how many there are.  Words without a meaning are zero, and so is all of v
 * beside a status that is not SPNG_DONE. */
enum { SPNG_SCOPE_NONE = 0,                     /* no parser here: IDAT, IEND, CgBI, tEXt / zTXt / iTXt / iCCP (their heads are the
                                                   directory's), private chunks */
       SPNG_SCOPE_PARSED = 1,                   /* the parser ran: status and values are its answer */
       SPNG_SCOPE_NO_HEADER = 2,                /* the file's IHDR is not where it must be, or did not parse: no parser behind it ran */
       SPNG_SCOPE_NO_PALETTE = 3 };             /* hIST, or bKGD / tRNS of an indexed image, with no PLTE that parsed in front of it (the
                                                   reference throws DecodingError.required(PLTE, before:): the host's rule) */
typedef struct spng_chunk_value {               /* 64 bytes */
    int32_t  status;                            /* SPNG_DONE or one of SPNG_E_PARSE_* */
    uint32_t scope;
    uint64_t aux[2];
    uint32_t count;                             /* PLTE: entries; indexed tRNS: alphas; hIST: entries; sPLT: entries */
    uint32_t k;                                 /* sPLT: payload offset of the NUL behind the name, else SPNG_NO_OFFSET */
    uint32_t v[8];
} spng_chunk_value;
typedef struct spng_parsed {                    /* per file */
    int32_t  status;                            /* of the first record in file order whose status is not SPNG_DONE (SPNG_DONE: none) */
    uint32_t index;                             /* ... and its index (SPNG_NO_OFFSET: none) */
    uint64_t aux[2];
    uint32_t ihdr_index, plte_index;            /* SPNG_NO_OFFSET: none among the entries */
    uint32_t palette_count;                     /* of that PLTE if it parsed, else 0 */
    uint8_t  depth, color, ios, interlaced;     /* of the header if it parsed, else 0 (ios: entry 0 is CgBI) */
} spng_parsed;
/* files, dirs, d_infos: exactly what spng_lex_dir_batch consumed and produced, still on the device; the entries a file has are
 * min(d_infos[i].chunks, dirs[i].cap).  d_values[i]: device memory for dirs[i].cap records, 8-byte aligned (NULL with a cap of 0);
 * records behind the entries stay untouched.  d_parsed / h_parsed: a record per file; with d_parsed alone the call is asynchronous on the context's
 * stream, and nothing waits between it and a spng_lex_dir_batch in front of it.  A wave per chunk; an sPLT's frequencies are
 * compared 64 entries per step.  SPNG_E_ARGUMENT (the call): a null array with a non-zero count, a null d_values[i] or a null
 * d_entries with a non-zero cap. */
int32_t spng_parse_dir_batch(spng_ctx *ctx, const spng_file_desc *files, const spng_chunk_dir *dirs, const spng_lexed *d_infos,
                             spng_chunk_value *const *d_values, uint32_t count, spng_parsed *d_parsed, spng_parsed *h_parsed);

/* ---- text: the byte work between a text chunk's body and a String ------------------------------------------------ */
enum { SPNG_TEXT_LATIN1_TO_UTF8 = 1,  /* String(uncompressed.map{ Character(Unicode.Scalar($0)) }).utf8 (PNG.Text.swift:198): a byte >= 0x80
                                         becomes (0xc0 | b >> 6, 0x80 | b & 0x3f) */
       SPNG_TEXT_CHECK_UTF8 = 2 };    /* is the input well-formed UTF-8 (Unicode 15, table 3-7)?  Nothing is written */
typedef struct spng_text_desc {
    const void *d_in;   uint64_t len;           /* device pointers of any alignment */
    void       *d_out;  uint64_t out_cap;       /* SPNG_TEXT_CHECK_UTF8: unused */
    uint8_t     op;
    uint8_t     reserved[7];                    /* zero */
} spng_text_desc;
/* Results.  SPNG_TEXT_LATIN1_TO_UTF8: SPNG_DONE, consumed = len, written = len + the number of bytes >= 0x80; or
 * SPNG_E_OUTPUT_CAPACITY with written = the bytes needed, nothing written.  SPNG_TEXT_CHECK_UTF8: SPNG_DONE, consumed = len,
 * written = 0; or SPNG_E_TEXT_ENCODING with aux[0] = the offset of the first ill-formed sequence and aux[1] = the number of bytes
 * that begin one -- sequences as a decoder that replaces maximal subparts finds them (Unicode 15, 3.9, U+FFFD substitution; what
 * Python's bytes.decode("utf-8", "replace") and Swift's String(decoding:as:) put a U+FFFD for): an overlong form, a surrogate, a
 * value above U+10FFFF, a stray or missing continuation byte, a sequence the end cuts off.  The input goes in tiles of 4096 bytes --
 * a count per tile, a scan over the tiles, the write --, so one long text runs on many workgroups.  A len of 0 is valid (and
 * well-formed).  SPNG_E_ARGUMENT (the call): an unknown op, a non-zero reserved byte, a null input with a len, a null output with an
 * out_cap (a null output with an out_cap of 0 asks for the bytes needed), input and output that overlap. */
int32_t spng_text_batch(spng_ctx *ctx, const spng_text_desc *descs, uint32_t count, spng_result *d_results, spng_result *h_results);

/* One zlib stream to cut into IDAT chunks of chunk_bytes payload bytes (the last one shorter). */
typedef struct spng_chunking_desc {
    const void *d_stream; uint64_t len;
    void       *d_out;    uint64_t out_cap;     /* len + 12 * ceil(len / chunk_bytes) bytes are written */
    uint64_t    chunk_bytes;
} spng_chunking_desc;
/* replaces PNG.BytestreamDestination.format(type: .IDAT, data:) for every chunk PNG.Encoder.pull returns
 * (Sources/PNG/Lexing/PNG.BytestreamDestination.swift:66-88, PNG.Image.swift:658-665). */
int32_t spng_write_idat_batch(spng_ctx *ctx, const spng_chunking_desc *descs, uint32_t count,
                              spng_result *d_results, spng_result *h_results);
/* CRC-32 of a host buffer computed on the device (swift-hash CRC32 as used by chunk()) */
int32_t spng_crc32(spng_ctx *ctx, const void *data, uint64_t n, uint32_t *out);

/* ---- files: whole PNG files written on the device ------------------------------------------------------ */
/* An ancillary chunk the caller hands over as it is: the writer frames it (length, type, CRC-32) and neither interprets nor
 * reorders it.  type: the four characters big-endian ('g' << 24 | 'A' << 16 | 'M' << 8 | 'A'); data: `len` HOST bytes. */
typedef struct spng_blob {
    uint32_t    type;
    uint32_t    len;
    const void *data;
} spng_blob;
/* One PNG file to write: signature, the head PNG.Image.compress writes in front of the image data, the zlib stream cut into IDAT
 * chunks, IEND.  The head, in the order of Sources/PNG/PNG.Image.swift:589-656:
 *   CgBI (bgr8: [48, 0, 32, 6], bgra8: [48, 0, 32, 2]; PNG.Image.swift:416-423), IHDR (PNG.Header.serialized, Parsing/PNG.Header.swift:133-145),
 *   the blobs of `before` (the reference's cHRM gAMA sRGB iCCP sBIT), PLTE, bKGD, tRNS (PNG.Layout.palette / .background /
 *   .transparency, Formats/PNG.Layout.swift:60-194), the blobs of `after` (hIST pHYs tIME iTXt sPLT and application chunks).
 * The format is named as in spng_unpack_desc: depth, channels, indexed, bgr.  palette: palette_count x (r, g, b, a) HOST bytes --
 * an indexed format's palette with its alphas (PLTE holds the colours; tRNS the alphas up to the last one that is not 255 and is
 * absent when all are), or the suggested palette of a colour format (PLTE only when it is not empty; the alphas are ignored).
 * key / fill: as PNG.Format holds them -- one field for the grey formats, (r, g, b), and (b, g, r) for bgr8 / bgra8, which the layout
 * turns back (PNG.Format.swift:427-430, PNG.Layout.swift:120-121, 176-178); fields of the 8-bit formats are at most 255 and are
 * widened to 16-bit big-endian ones; an indexed format's fill is fill[0], a palette index.
 * The stream: d_stream[0 .. n) with n = stream_len, or -- d_stream_result given -- n = d_stream_result->written, read on the
 * device: the slot spng_encode_batch / spng_deflate_batch wrote with d_results, so that nothing waits between the two calls.
 * stream_cap: a host-known bound on n (the capacity of d_stream; spng_deflate_bound is the natural value); it sizes the launch.  With
 * a host length it may be 0 (= stream_len). */
typedef struct spng_png_desc {
    const void        *d_stream;  uint64_t stream_len;
    const spng_result *d_stream_result;         /* device pointer, or NULL: stream_len holds.  Must not lie in the call's d_results */
    uint64_t           stream_cap;
    void              *d_out;     uint64_t out_cap;     /* spng_file_bound(desc, n) bytes are written */
    uint64_t           chunk_bytes;             /* payload bytes of every IDAT but the last: 1 ... 0x7fffffff.  The reference cuts at twice
                                                   the capacity its output buffer got (LZ77.DeflatorOut.swift:15-24, 121): an allocator
                                                   fact, 65544 at the default hint on Linux, 8200 at hint 4096 */
    uint32_t           width, height;
    uint8_t            depth, channels, indexed, bgr, interlaced, has_key, has_fill, reserved;   /* reserved: zero */
    uint16_t           key[3], fill[3];
    uint32_t           palette_count;
    const uint8_t     *palette;
    const spng_blob   *before;    uint32_t before_count;
    const spng_blob   *after;     uint32_t after_count;
} spng_png_desc;
/* The exact size of the file for a stream of stream_len bytes: 8 + head + stream_len + 12 ceil(stream_len / chunk_bytes) + 12 --
 * with spng_deflate_bound the capacity to allocate.  0: a desc spng_write_file_batch refuses, or stream_len == 0. */
uint64_t spng_file_bound(const spng_png_desc *desc, uint64_t stream_len);
/* replaces PNG.Image.compress(stream:level:hint:) behind its encoder (Sources/PNG/PNG.Image.swift:576-668): signature(), the format(type:data:)
 * of every chunk (Lexing/PNG.BytestreamDestination.swift:44-88) and the IDAT loop -- every chunk but the last carries chunk_bytes
 * bytes, and none is empty (the last pull() of an exhausted stream returns nil, LZ77.DeflatorBuffers.swift:142-151).  Lengths, types
 * and CRC-32s of the head are laid down on the host and uploaded with the job table; payloads move and are summed on the device, a
 * chunk longer than 1 MiB in pieces of 1 MiB by a wave each.  Refused with SPNG_E_ARGUMENT (the call; nothing is launched): a blob
 * whose type is CgBI IHDR PLTE bKGD tRNS IDAT IEND or one spng_lex_batch would not accept (PNG.Chunk.swift:69-88), a palette count
 * outside what the format allows (PNG.Format.swift:274-309), a width or height of 0, chunk_bytes outside 1 ... 0x7fffffff, a depth /
 * channels / flag combination that is no PNG.Format, a key where the format has none, a field its format does not hold.
 * Results per file: SPNG_DONE with written = file bytes, consumed = stream bytes, aux[0] = IDAT chunks.  SPNG_E_OUTPUT_CAPACITY
 * with written = the bytes needed, nothing written.  A source result whose status is not SPNG_DONE: that status and its aux,
 * written = consumed = 0, nothing written.  SPNG_E_ARGUMENT: n == 0 (no zlib stream is empty) or n > stream_cap.
 * With d_results only the call stays asynchronous. */
int32_t spng_write_file_batch(spng_ctx *ctx, const spng_png_desc *descs, uint32_t count,
                              spng_result *d_results, spng_result *h_results);
/* replaces PNG.Image.compress(stream:level:hint:) from storage (PNG.Image.swift:576-668): spng_encode_batch over `images`, then the
 * writer over `files` reading the encoder's results on the device -- no host wait between them, one optional read-back.  images[i]:
 * as for spng_encode_batch (d_idat / idat_len: where the stream goes and its capacity).  files[i]: d_out, out_cap, chunk_bytes,
 * indexed, bgr, palette, key, fill and the blobs; its stream fields, width, height, depth, channels and interlaced are taken from
 * images[i] (bgr must agree with images[i].format == SPNG_FORMAT_IOS).  Formats, sizes, interlacing and standards may be mixed. */
int32_t spng_compress_batch(spng_ctx *ctx, const spng_image_desc *images, const spng_png_desc *files, int32_t level, uint32_t count,
                            spng_result *d_results, spng_result *h_results);

/* A stream that arrives in pieces (PNG.Context.push(data:) per IDAT chunk): defilters and assigns the
 * scanlines that became complete between h_prev_len[i] and h_now_len[i] inflated bytes -- what PNG.Decoder.row / pass keep
 * track of (Sources/PNG/Decoding/PNG.Decoder.swift:20-21, 88-94, 121-135) -- each row once, with the defiltered row above it
 * as an earlier call left it (in d_storage for 8 / 16-bit non-interlaced images; in d_work[i], a buffer of the size and layout
 * of d_rows, for interlaced and sub-byte ones: d_rows itself stays as inflated, it is the LZ77 window of the next push).
 * results: written = scanline bytes defiltered by this call, consumed = inflated bytes that are whole rows by now.
 * descs[i].reserved & SPNG_IMAGE_OVERDRAW: push(data:overdraw: true) -- see SPNG_IMAGE_OVERDRAW. */
int32_t spng_unfilter_resume_batch(spng_ctx *ctx, const spng_image_desc *descs, void *const *d_work,
                                   const uint64_t *h_prev_len, const uint64_t *h_now_len, uint32_t count,
                                   spng_result *d_results, spng_result *h_results);

/* ---- pixels: the step behind the decode path ----------------------------------------------------- */
/* One image to unpack.  palette: indexed formats only, palette_count x 4 bytes (r, g, b, a): PLTE with the
 * tRNS alphas folded in, as PNG.Format keeps it.  key: the chroma key of a v / rgb / bgr format as PNG.Format keeps it, compared with
 * the samples in the order they lie in storage (PNG.RGBA.swift:318-323): (v), (r, g, b), and (b, g, r) for bgr8 -- a CgBI file's tRNS
 * key, which is (r, g, b), REVERSED, as the reference does when it builds the format (PNG.Format.swift:427-430). */
typedef struct spng_unpack_desc {
    const void *d_storage;                      /* PNG.Image.storage, S bytes                        */
    void       *d_out;                          /* width * height RGBA quadruplets of `target` bits, at a multiple of T
                                                   (target / 8 bytes: any address for UInt8, an even one for UInt16 -- as
                                                   spng_pack_desc.d_pixels; SPNG_E_ARGUMENT otherwise).  d_storage: any address */
    const void *d_palette;
    uint32_t    width, height;
    uint32_t    palette_count;
    uint16_t    key[3];
    uint8_t     depth, channels;                /* as in spng_image_desc                             */
    uint8_t     indexed;                        /* PNG.Format.indexed1/2/4/8                         */
    uint8_t     bgr;                            /* PNG.Format.bgr8 / bgra8 (CgBI)                    */
    uint8_t     has_key;
    uint8_t     target;                         /* 8 or 16: T = UInt8 / UInt16                        */
    uint8_t     layout;                         /* SPNG_TARGET_RGBA: PNG.RGBA<T>, SPNG_TARGET_VA: PNG.VA<T> (v = the grey value or
                                                   the red channel, a) -- d_out holds width * height (v, a) pairs then;
                                                   SPNG_TARGET_SCALAR: T, the scalar unpack of PNG.Image.swift:682-760, 1030-1040
                                                   (grey value / red channel / palette[i].r; keys ignored, no premultiply) */
    uint8_t     premultiply;                    /* 0: straight;  SPNG_PREMULTIPLY: .premultiplied (PNG.RGBA.swift:121-127,
                                                   PNG.VA.swift:57-60);  SPNG_PREMULTIPLY_AS_U8 (target 16 only):
                                                   .premultiplied(as: UInt8.self) (PNG.RGBA.swift:146-158), the form the
                                                   reference's iOS goldens are compared in (Roundtripping.swift:206-215);
                                                   SPNG_STRAIGHTEN / SPNG_STRAIGHTEN_AS_U8 (target 16 only): .straightened /
                                                   .straightened(as: UInt8.self) -- unpack(as:).map(\.straightened), the first step of
                                                   Snippets/PNG/iPhoneOptimized.swift, in one pass.  A component the reference
                                                   traps on is written as T.max silently here: spng_alpha_batch is the entry
                                                   that counts them */
    uint8_t     reserved[6];
} spng_unpack_desc;
enum { SPNG_TARGET_RGBA = 0, SPNG_TARGET_VA = 1, SPNG_TARGET_SCALAR = 2 };
enum { SPNG_PREMULTIPLY = 1,          /* .premultiplied                  (PNG.RGBA.swift:121-127, PNG.VA.swift:57-60)    */
       SPNG_PREMULTIPLY_AS_U8 = 2,    /* .premultiplied(as: UInt8.self)  (PNG.RGBA.swift:146-158), T = UInt16 only       */
       SPNG_STRAIGHTEN = 3,           /* .straightened                   (PNG.RGBA.swift:167-173, PNG.VA.swift:98-101)   */
       SPNG_STRAIGHTEN_AS_U8 = 4 };   /* .straightened(as: UInt8.self)   (PNG.RGBA.swift:192-206), T = UInt16 only       */
/* replaces PNG.RGBA<T>.unpack(_:of:deindexer:) / PNG.VA<T>.unpack(_:of:deindexer:) with the default deindexers, T = UInt8 / UInt16
 * (Sources/PNG/ColorTargets/PNG.RGBA.swift:259-365, depth rescaling Sources/PNG/PNG.swift:255-312,
 * 495-524; PNG.VA.swift:184-290; premultiplication PNG.swift:55-66); what PNG.Image.unpack(as:) returns.  All descs
 * of a call share `target`.  Output: r, g, b, a (or v, a) per pixel in host byte order. */
int32_t spng_unpack_batch(spng_ctx *ctx, const spng_unpack_desc *descs, uint32_t count);
int32_t spng_unpack(spng_ctx *ctx, const void *storage, uint32_t w, uint32_t h, int depth, int channels,
                    int indexed, int bgr, int target, const void *palette, uint32_t palette_count,
                    const uint16_t *key, void *out);
/* the same with a colour-target layout (SPNG_TARGET_*) and premultiplication (0 / SPNG_PREMULTIPLY*) */
int32_t spng_unpack_as(spng_ctx *ctx, const void *storage, uint32_t w, uint32_t h, int depth, int channels,
                       int indexed, int bgr, int target, int layout, int premultiply, const void *palette,
                       uint32_t palette_count, const uint16_t *key, void *out);

/* ---- pixels: the step in front of the encode path ------------------------------------------------ */
/* One image to pack: the inverse of spng_unpack_desc.  d_pixels: width * height RGBA<T> quadruplets (r, g, b, a), VA<T> pairs
 * (v, a) or scalars T in host byte order, T = UInt8 / UInt16 (`source` bits); d_storage: PNG.Image.storage, S bytes. */
typedef struct spng_pack_desc {
    const void *d_pixels;
    void       *d_storage;
    const void *d_palette;                      /* indexed formats: palette_count x (r, g, b, a), as in spng_unpack_desc */
    uint32_t    width, height;
    uint32_t    palette_count;
    uint8_t     depth, channels;                /* as in spng_image_desc                             */
    uint8_t     indexed;                        /* PNG.Format.indexed1/2/4/8                         */
    uint8_t     bgr;                            /* PNG.Format.bgr8 / bgra8 (CgBI)                    */
    uint8_t     source;                         /* 8 or 16: T = UInt8 / UInt16                        */
    uint8_t     layout;                         /* SPNG_TARGET_RGBA / _VA / _SCALAR                   */
    uint8_t     premultiply;                    /* 0: as they are;  SPNG_PREMULTIPLY;  SPNG_PREMULTIPLY_AS_U8 (source 16 only): the
                                                   components are premultiplied before they are narrowed, indexed and swizzled --
                                                   pack(pixels.map(\.premultiplied)), the last step of Snippets/PNG/iPhoneOptimized.swift,
                                                   in one pass (an indexed format looks up the premultiplied colour).  Not with
                                                   SPNG_TARGET_SCALAR */
    uint8_t     reserved[5];
} spng_pack_desc;
/* replaces PNG.RGBA<T>.pack(_:as:indexer:) / PNG.VA<T>.pack(_:as:indexer:) / the scalar PNG.Image.pack<T> with the default
 * indexers, T = UInt8 / UInt16 -- what PNG.Image.init(packing:size:layout:) stores (Sources/PNG/ColorTargets/PNG.RGBA.swift:409-478,
 * PNG.VA.swift:334-403, PNG.Image.swift:767-834, 935-1010, 1043-1062; depth rescaling PNG.deconvolve, Sources/PNG/PNG.swift:699-1285;
 * default indexers PNG.Color.swift:158-226).  Components of T are narrowed to the format's depth by a right shift or widened by
 * the quantum, stored big-endian; colour formats without alpha drop it; chroma keys play no part.  Indexed formats: the palette
 * entry equal to the pixel reduced to 8 bits, entry 0 when there is none (the reference traps on a palette that holds a colour
 * twice; here the lowest index wins).  All descs of a call share `source`.  The storage can go straight to spng_encode_batch. */
int32_t spng_pack_batch(spng_ctx *ctx, const spng_pack_desc *descs, uint32_t count);
/* host-pointer convenience (copies in / out, synchronous) */
int32_t spng_pack_as(spng_ctx *ctx, const void *pixels, uint32_t w, uint32_t h, int depth, int channels,
                     int indexed, int bgr, int source, int layout, const void *palette, uint32_t palette_count, void *storage);

/* ---- pixels: premultiplied and straight alpha ------------------------------------------------------ */
/* One array of colour-target pixels to premultiply or straighten.  Both pointers are device pointers aligned to T. */
typedef struct spng_alpha_desc {
    const void *d_in;  void *d_out;             /* `count` pixels each; d_out == d_in is allowed (in place), any other overlap is not */
    uint64_t    count;
    uint8_t     bits;                           /* 8 or 16: T = UInt8 / UInt16; all descs of a call share it */
    uint8_t     layout;                         /* SPNG_TARGET_RGBA: (r, g, b, a) or SPNG_TARGET_VA: (v, a) */
    uint8_t     op;                             /* SPNG_PREMULTIPLY ... SPNG_STRAIGHTEN_AS_U8 (the _AS_U8 forms: bits 16 only) */
    uint8_t     reserved[5];                    /* zero */
} spng_alpha_desc;
/* replaces PNG.RGBA<T>.premultiplied / .straightened and their (as: UInt8.self) forms, and the same of PNG.VA<T>, mapped over an
 * array (Sources/PNG/ColorTargets/PNG.RGBA.swift:121-206, PNG.VA.swift:57-131; PNG.premultiply / PNG.straighten,
 * Sources/PNG/PNG.swift:55-117), bit for bit, with M = T.max:
 *   premultiply   (c * a + (M >> 1)) / M;            straighten   a == 0 ? p : (M * p + (a >> 1)) / a;       alpha as it is
 *   the _AS_U8 forms: every component, alpha included, shifted right by 8, the operation at M = 255, every component times 257.
 * Where the reference traps -- a > 0 and p > a, compared after the shift in the _AS_U8 form: the quotient does not fit T -- the
 * component becomes T.max (255 * 257 in the _AS_U8 form).  Results: status SPNG_DONE, written = bytes written, aux[0] = the
 * number of such components.  A count of 0, of a desc or of the call, is valid and writes nothing. */
int32_t spng_alpha_batch(spng_ctx *ctx, const spng_alpha_desc *descs, uint32_t count,
                         spng_result *d_results, spng_result *h_results);
/* host-pointer convenience (copies in / out, synchronous): n pixels */
int32_t spng_alpha(spng_ctx *ctx, const void *pixels, uint64_t n, int bits, int layout, int op, void *out, spng_result *result);

/* ---- pixels: a custom colour target (the HSVA tutorial) --------------------------------------------- */
/* The reference's third colour-target tutorial (Snippets/PNG/CustomColor.swift) defines its own target,
 *     struct HSVA { var h:UInt32, s:UInt16, v:UInt8, a:UInt8 }           -- in memory {uint32 h; uint16 s; uint8 v; uint8 a}:
 * 8 bytes, aligned to 4, host byte order --, unpacks an image into it, edits the fields and packs the result.  Its three
 * conversions, mapped over an array, bit for bit (all arithmetic in UInt32; (min, mid, max) the sorted r, g, b; d = max - min):
 *   SPNG_HSVA_FROM_RGBA8   HSVA.init(r:g:b:a:), CustomColor.swift:19-49.  sector from (r < g, g < b, r < b) as the switch orders
 *                          them ((false, false, _) is sector 0).  d > 0: f = ((mid - min) << 16) / d + 1, h = 65537 sector +
 *                          (sector even ? f : 65537 - f), s = ((d << 16) - 1) / max; d == 0: h = s = 0.  v = max, a as it is.
 *   SPNG_HSVA_TO_RGBA8     HSVA.rgba, CustomColor.swift:51-78.  s == 0 or v == 0: (v, v, v, a).  Otherwise (sector, r') = h divmod
 *                          65537, f = sector even ? r' : 65537 - r', d = ((s v) >> 16) + 1, x = v, y = x - d, z = ((f d) >> 16) + y,
 *                          and (r, g, b) = (x, z, y), (z, x, y), (y, x, z), (y, z, x), (z, y, x), (x, y, z) for sector 0 ... 5.
 *   SPNG_HSVA_TO_VA8       (v, a): what HSVA.pack stores for the grey formats (kernel: \.v, CustomColor.swift:232-251) -- not .rgba.r.
 * TO_RGBA8(FROM_RGBA8(c)) == c for every colour.  Where the reference traps -- only fatalError("unreachable"): sector >= 6 with
 * s > 0 and v > 0 -- the pixel becomes (v, v, v, a) and is counted in spng_result.aux[0], as spng_alpha_batch counts its own.
 *
 * Two steps make HSVA.unpack (CustomColor.swift:86-210): for every PNG.Format it equals FROM_RGBA8 applied to
 * RGBA<UInt8>.unpack (spng_unpack_batch, target 8, SPNG_TARGET_RGBA; Sources/PNG/ColorTargets/PNG.RGBA.swift:259-365) -- the colour
 * formats hand init(r:g:b:a:) the very components RGBA<UInt8> holds; the grey formats store (h: 0, s: 0, v, a), which is what
 * (v, v, v, a) converts to (no comparison holds: sector 0, d = 0); chroma keys and palettes (deindexers included) are resolved by
 * the existing unpack.  HSVA.pack (CustomColor.swift:213-299) by the format packed into:
 *   grey (v1 ... v16, va8, va16)      TO_VA8,   then spng_pack_batch with source 8, SPNG_TARGET_VA
 *   colour (rgb*, bgr8, rgba*, bgra8) TO_RGBA8, then spng_pack_batch with source 8, SPNG_TARGET_RGBA
 *   indexed                           TO_RGBA8, then the indexed path of spng_pack_batch, or spng_census_batch +
 *                                     spng_pack_indexed_batch for a custom indexer
 * The price of not fusing the conversion into the unpack and pack kernels is one more pass over 4 bytes per pixel. */
enum { SPNG_HSVA_FROM_RGBA8 = 1, SPNG_HSVA_TO_RGBA8 = 2, SPNG_HSVA_TO_VA8 = 3 };
typedef struct spng_hsva_desc {
    const void *d_in;  void *d_out;             /* device pointers to `count` pixels each.  The HSVA side is aligned to 4; the
                                                   RGBA8 / VA8 side may have any alignment (16 on both sides is the fast path) */
    uint64_t    count;
    uint8_t     op;                             /* SPNG_HSVA_FROM_RGBA8 ... SPNG_HSVA_TO_VA8; every desc has its own */
    uint8_t     reserved[7];                    /* zero */
} spng_hsva_desc;
/* Results: status SPNG_DONE, written = bytes written, consumed = bytes read, aux[0] = pixels the reference would have trapped on.
 * A count of 0, of a desc or of the call, is valid and writes nothing.  SPNG_E_ARGUMENT: a non-zero reserved byte, an unknown op,
 * d_out == d_in (the element sizes differ, so nothing runs in place) or any other overlap, an HSVA pointer not aligned to 4. */
int32_t spng_hsva_batch(spng_ctx *ctx, const spng_hsva_desc *descs, uint32_t count,
                        spng_result *d_results, spng_result *h_results);
/* host-pointer convenience (copies in / out, synchronous): n pixels */
int32_t spng_hsva(spng_ctx *ctx, const void *pixels, uint64_t n, int op, void *out, spng_result *result);

/* ---- pixels: the luminance of the BasicEncoding tutorial ---------------------------------------------- */
/* The pixel step of the reference's tutorial Snippets/PNG/BasicEncoding.swift, COMPUTE_LUMINANCE (:63-71), mapped over an array of
 * RGBA<UInt8> (PNG.Image.init(packing: rgba, layout: .v8) itself keeps only r, which is why the tutorial converts first):
 *     let l:Double = (0.299 * r * r + 0.587 * g * g + 0.114 * b * b).squareRoot()
 *     return .init(max(0, min(l.rounded(), 255)))
 * bit for bit: IEEE-754 binary64, every product and sum rounded on its own in the association
 * x = ((0.299 r) r + (0.587 g) g) + (0.114 b) b, the correctly rounded root of x, rounded to the nearest integer with halves away
 * from zero (Swift's .rounded()), clamped to 0 ... 255.  (Of the 2^24 colours 38 land on an exact half, 97 differ when evaluated in
 * float, 2 when the products are associated the other way.)  Nothing here can trap in the reference -- the clamp is part of the
 * formula -- so aux[0] is always 0.
 *   SPNG_LUMINANCE_V8    -> UInt8: the tutorial's [UInt8], ready for spng_pack_batch with source 8, SPNG_TARGET_SCALAR
 *   SPNG_LUMINANCE_VA8   -> (l, a): the same l with the pixel's alpha, ready for SPNG_TARGET_VA */
enum { SPNG_LUMINANCE_V8 = 1, SPNG_LUMINANCE_VA8 = 2 };
typedef struct spng_luminance_desc {
    const void *d_in;  void *d_out;             /* device pointers to `count` pixels each: RGBA<UInt8> in, UInt8 or (UInt8, UInt8)
                                                   out.  Any alignment (16 on both sides is the fast path) */
    uint64_t    count;
    uint8_t     op;                             /* SPNG_LUMINANCE_V8 or SPNG_LUMINANCE_VA8; every desc has its own */
    uint8_t     reserved[7];                    /* zero */
} spng_luminance_desc;
/* Results: status SPNG_DONE, written = bytes written, consumed = bytes read, aux[0] = 0.  A count of 0, of a desc or of the call, is
 * valid and writes nothing.  SPNG_E_ARGUMENT: a non-zero reserved byte, an unknown op, a null pointer with a non-zero count,
 * d_out == d_in (the element sizes differ, so nothing runs in place) or any other overlap, a count whose byte size overflows. */
int32_t spng_luminance_batch(spng_ctx *ctx, const spng_luminance_desc *descs, uint32_t count,
                             spng_result *d_results, spng_result *h_results);
/* host-pointer convenience (copies in / out, synchronous): n pixels */
int32_t spng_luminance(spng_ctx *ctx, const void *pixels, uint64_t n, int op, void *out, spng_result *result);

/* ---- pixels: indexed colour with any pure indexer ---------------------------------------------------- */
/* The reference takes an indexer closure wherever pixels are packed into an indexed format:
 *   PNG.RGBA<T>.pack(_:as:indexer:)  ((UInt8, UInt8, UInt8, UInt8)) -> Int   Sources/PNG/ColorTargets/PNG.RGBA.swift:409-423
 *   PNG.VA<T>.pack(_:as:indexer:)    ((UInt8, UInt8)) -> Int                 PNG.VA.swift:334-350
 *   PNG.Image.pack<T>(_:as:indexer:) (UInt8) -> Int                          Sources/PNG/PNG.Image.swift:767-782
 *   PNG.Image.init(packing:size:layout:metadata:indexer:)                    PNG.Image.swift:935-996
 *   PNG.deconvolve(_:_:dereference:), which hands the closure its argument   Sources/PNG/PNG.swift:747-854
 * Every argument is a UInt8 aggregate, so a pure closure is a table.  The KEY of a pixel is that aggregate as 32 bits: the
 * components after the optional premultiplication, reduced to UInt8 as PNG.deconvolve does (PNG.swift:829-852: as they are for
 * T = UInt8, >> 8 for T = UInt16),
 *     RGBA: r | g << 8 | b << 16 | a << 24        VA: v | a << 8        scalar: v
 * spng_census_batch reports the distinct keys of a pixel array (and how often each occurs: the frequencies of PNG.Histogram and
 * of sPLT entries); the host evaluates the indexer once per key; spng_pack_indexed_batch stores the index of every pixel.  The
 * storage can go straight to spng_encode_batch: the pixels never leave the device. */
typedef struct spng_census_desc {
    const void *d_pixels;                       /* `count` pixels, aligned to T */
    uint64_t    count;
    void       *d_keys;                         /* cap x uint32 */
    void       *d_counts;                       /* cap x uint64, or NULL */
    uint32_t    cap;                            /* 1 ... 65536 */
    uint8_t     bits;                           /* 8 or 16: T = UInt8 / UInt16; all descs of a call share it */
    uint8_t     layout;                         /* SPNG_TARGET_RGBA / _VA / _SCALAR */
    uint8_t     premultiply;                    /* 0, SPNG_PREMULTIPLY or SPNG_PREMULTIPLY_AS_U8 (bits 16 only), as in spng_pack_desc:
                                                   the keys of pixels.map(\.premultiplied).  Not with SPNG_TARGET_SCALAR */
    uint8_t     reserved[1];                    /* zero */
} spng_census_desc;
/* At most `cap` distinct keys: status SPNG_DONE, written = their number n, consumed = count; d_keys[0 .. n) hold them in ascending
 * order, d_counts[i] how many pixels have key i (the counts sum to `count`); both arrays are left untouched behind n.  More than
 * `cap`: status SPNG_E_OUTPUT_CAPACITY, written = 0, the contents of both arrays unspecified (the kernel stops reading the
 * pixels once it knows).  A count of 0 is valid: SPNG_DONE, written = 0.  The output is a function of the pixels alone -- never of
 * the batch an array travels in, the launch or the run.  Scratch of the context: 16 bytes per slot of a table of 2 x cap slots
 * (rounded up to a power of two) and 8 per key for the sort, per array of the call; spng_trim gives it back. */
int32_t spng_census_batch(spng_ctx *ctx, const spng_census_desc *descs, uint32_t count,
                          spng_result *d_results, spng_result *h_results);
/* host-pointer convenience (copies in / out, synchronous): n pixels; keys: cap x uint32; counts: cap x uint64 or NULL */
int32_t spng_census(spng_ctx *ctx, const void *pixels, uint64_t n, int bits, int layout, int premultiply, uint32_t cap,
                    uint32_t *keys, uint64_t *counts, spng_result *result);

typedef struct spng_pack_indexed_desc {
    const void *d_pixels;                       /* width * height pixels, aligned to T */
    void       *d_storage;                      /* one byte per pixel, any alignment: PNG.Image.storage of an indexed8 image, as the
                                                   indexed path of spng_pack_batch writes it */
    const void *d_keys;                         /* map_count x uint32, ASCENDING AND DISTINCT: the form the census writes */
    const void *d_indices;                      /* map_count bytes: the indexer's result for each key */
    uint32_t    width, height;
    uint32_t    map_count;                      /* 0 ... 65536 */
    uint8_t     source;                         /* 8 or 16: T = UInt8 / UInt16; all descs of a call share it */
    uint8_t     layout, premultiply;            /* as in spng_census_desc */
    uint8_t     miss;                           /* stored for a pixel whose key is not in d_keys */
    uint8_t     reserved[8];                    /* zero */
} spng_pack_indexed_desc;
/* Every pixel stores d_indices[j] where d_keys[j] equals its key, and `miss` where none does.  Results: status SPNG_DONE,
 * written = pixels, aux[0] = pixels that missed.  Keys that are not ascending and distinct are the caller's responsibility here
 * (device memory is not looked at by the host; the lookup may then miss keys that are present, nothing worse); the host-pointer
 * form below sees them and returns SPNG_E_ARGUMENT. */
int32_t spng_pack_indexed_batch(spng_ctx *ctx, const spng_pack_indexed_desc *descs, uint32_t count,
                                spng_result *d_results, spng_result *h_results);
/* host-pointer convenience (copies in / out, synchronous) */
int32_t spng_pack_indexed(spng_ctx *ctx, const void *pixels, uint32_t w, uint32_t h, int source, int layout, int premultiply,
                          const uint32_t *keys, const uint8_t *indices, uint32_t map_count, int miss, void *storage,
                          spng_result *result);

/* ---- pixels: colour tables without a ceiling ----------------------------------------------------------- */
/* The reference lets a caller put ANY pure function between pixels and storage: the indexer closures above
 * (PNG.RGBA.swift:409-423, PNG.VA.swift:334-350, PNG.Image.swift:767-782, 935-996) and whole colour targets of the caller's own
 * (Snippets/PNG/CustomColor.swift).  A pure function of a UInt8 aggregate is a table; the two entries above stop at 65 536 keys and
 * at one byte per result, these two do not: spng_census_wide_batch reports up to 2^24 distinct keys, the host evaluates the
 * function once per key, spng_map_batch stores its result -- 1, 2, 4 or 8 bytes -- for every pixel.  A photographic RGBA image
 * through a nearest-palette indexer, or the CustomColor tutorial's HSVA target (97 388 colours in its picture), is a census, one
 * vectorised host function over the keys, and a map.
 *
 * spng_census_wide_batch: the desc, the key and the output contract of spng_census_batch, with cap = 1 ... SPNG_CENSUS_WIDE_CAP.
 * Keys ascending with their 64-bit counts, both arrays untouched behind `written`; more than cap keys: SPNG_E_OUTPUT_CAPACITY with
 * written = 0; a count of 0 is valid; the output is a function of the pixels alone, and for any input spng_census_batch accepts
 * the bytes are the same.  Scratch of the context is sized by k = min(cap, count) per array, not by cap -- a caller who does not
 * know the number of colours passes cap = min(n, 2^24) --: 16 bytes per slot of a table of 2 k slots rounded up to a power of two
 * and 8 per element of a sort buffer of k rounded up to one, at most 80 bytes per key of k, plus 256 per array; spng_trim gives it
 * back.  The call WAITS once, for the counting kernel, to size the sort behind it by the keys found and not by cap (as
 * spng_deflate_batch waits for its probe kernel at levels >= 8); it is asynchronous from there on. */
enum { SPNG_CENSUS_WIDE_CAP = 16777216 };           /* 2^24 */
int32_t spng_census_wide_batch(spng_ctx *ctx, const spng_census_desc *descs, uint32_t count,
                               spng_result *d_results, spng_result *h_results);
/* host-pointer convenience (copies in / out, synchronous): n pixels; keys: min(cap, max(n, 1)) x uint32; counts: as many uint64, or NULL */
int32_t spng_census_wide(spng_ctx *ctx, const void *pixels, uint64_t n, int bits, int layout, int premultiply, uint32_t cap,
                         uint32_t *keys, uint64_t *counts, spng_result *result);

typedef struct spng_map_desc {                      /* 64 bytes */
    const void *d_pixels;                           /* `count` pixels, aligned to T */
    void       *d_out;                              /* `count` values of value_bytes, aligned to value_bytes */
    const void *d_keys;                             /* map_count x uint32, ASCENDING AND DISTINCT: the form the census writes */
    const void *d_values;                           /* map_count values, aligned to value_bytes: the function's result for each key */
    uint64_t    count;
    uint32_t    map_count;                          /* 0 ... SPNG_CENSUS_WIDE_CAP */
    uint8_t     source;                             /* 8 or 16: T = UInt8 / UInt16; all descs of a call share it */
    uint8_t     layout, premultiply;                /* as in spng_pack_indexed_desc */
    uint8_t     value_bytes;                        /* 1, 2, 4 or 8 */
    uint8_t     miss[8];                            /* the first value_bytes bytes: written for a pixel whose key is not in d_keys */
    uint8_t     reserved[8];                        /* zero */
} spng_map_desc;
/* Every pixel stores d_values[j] where d_keys[j] equals its key, and `miss` where none does.  Results: status SPNG_DONE, written =
 * bytes written, consumed = pixels, aux[0] = pixels that missed.  With value_bytes == 1 and map_count <= 65536 the bytes are those of
 * spng_pack_indexed_batch.  Keys that are not ascending and distinct are the caller's responsibility here (device memory is not
 * looked at by the host): the order does not matter to this entry, and a key present twice resolves to its LOWEST position --
 * deterministic, never a hang, never an access outside the arrays; the host-pointer form below sees such keys and returns
 * SPNG_E_ARGUMENT.  Scratch of the context, for maps above 512 keys: 8 bytes per slot of a table of 2 x map_count slots rounded up
 * to a power of two (at most 32 bytes per key); spng_trim gives it back. */
int32_t spng_map_batch(spng_ctx *ctx, const spng_map_desc *descs, uint32_t count,
                       spng_result *d_results, spng_result *h_results);
/* host-pointer convenience (copies in / out, synchronous): n pixels; values, miss and out hold items of value_bytes */
int32_t spng_map(spng_ctx *ctx, const void *pixels, uint64_t n, int source, int layout, int premultiply, const uint32_t *keys,
                 const void *values, uint32_t map_count, int value_bytes, const void *miss, void *out, spng_result *result);

/* ---- encode -------------------------------------------------------------------------------- */
/* replaces PNG.Encoder.filter (PNG.Encoder.swift:132-204) + PNG.Image.collect
 * (PNG.Image.swift:431-544): storage -> filtered rows with the reference's filter choice. */
int32_t spng_filter_batch(spng_ctx *ctx, const spng_image_desc *descs, uint32_t count,
                          spng_result *d_results, spng_result *h_results);
int32_t spng_filter(spng_ctx *ctx, const void *storage,
                    uint32_t w, uint32_t h, int depth, int channels, int interlaced,
                    void *rows, spng_result *result);

/* replaces LZ77.Deflator(format:level:exponent:hint:) push(all, last: true) + concatenated pull() output:
 * Sources/LZ77/Deflator/LZ77.Deflator.swift:8-44, LZ77.DeflatorBuffers.swift:46-93,
 * LZ77.DeflatorBuffers.Stream.swift:30-709, LZ77.DeflatorMatches.swift:225-379 (levels >= 8).  Every level of
 * LZ77.DeflatorSearch (:13-35) runs on the device: greedy 0-3, lazy 4-7, shortest path 8 and up (>= 13: the
 * last row).  `hint` only sizes the reference's output chunks (platform dependent there): the host re-chunks
 * the concatenated stream into IDATs of any size.  d_dst capacity: spng_deflate_bound(src_len).  The window
 * exponent travels in spng_stream_desc.reserved (batch form) / the `exponent` argument; PNG always uses 15,
 * and LZ77.Format.ios ignores it (LZ77.DeflatorBuffers.swift:52-55).  SPNG_FORMAT_GZIP: Gzip.Deflator (header, CRC-32 and
 * byte count of the input appended on the device).  Levels >= 8: the call waits for a small probe kernel (how
 * repetitive is each input: compressible streams get helper waves) before it enqueues the compression, so it is
 * asynchronous only from there on.
 * A capacity below the stream's length L (every format, the gzip trailer included): SPNG_E_OUTPUT_CAPACITY with written = L, the
 * bytes the whole stream needs -- allocate that much and call again --, consumed = src_len, and d_dst[0 .. dst_cap) = the stream's
 * first dst_cap bytes; nothing is stored behind dst_cap.  dst_cap may be 0 (d_dst must still be a pointer). */
uint64_t spng_deflate_bound(uint64_t n);
int32_t spng_deflate_batch(spng_ctx *ctx, const spng_stream_desc *descs, const int32_t *levels, uint32_t count,
                           spng_result *d_results, spng_result *h_results);
int32_t spng_deflate(spng_ctx *ctx, const void *src, uint64_t n, int32_t format, int32_t level,
                     void *dst, uint64_t cap, spng_result *result);
int32_t spng_deflate_window(spng_ctx *ctx, const void *src, uint64_t n, int32_t format, int32_t level, int32_t exponent,
                            void *dst, uint64_t cap, spng_result *result);
/* LZ77.Deflator.push(_:last:) for streams that arrive in pieces (Sources/LZ77/Deflator/LZ77.Deflator.swift:14-30; the reference
 * compresses whenever more than 4096 bytes are buffered, LZ77.DeflatorBuffers.swift:68-93, and its output does not depend on how
 * the input was pushed): d_src / src_len = ALL input bytes received so far (the caller appends to its device buffer), d_dst = the
 * stream so far, kept between calls.  d_states[i]: spng_deflate_state_bytes() bytes of device memory per stream, zero-filled
 * before the first push and left alone afterwards -- the device-side counterpart of LZ77.DeflatorBuffers.Stream (parse position,
 * queued terms, symbol costs, block limit, bit writer, checksum).  last[i] != 0: this is all the input.  A call emits what the
 * bytes so far determine: levels 0-7 every term whose positions see their whole 258-byte look-ahead, levels 8 and up every whole
 * block (2047, 4095, ... vertices); the rest waits for the next push.  Results: SPNG_NEED_MORE_INPUT with written = stream bytes
 * so far, consumed = input bytes parsed, aux = the host-side part of the state to hand to the next call as h_state[2 i], [2 i + 1]
 * (levels >= 8: it sizes the call's launches; NULL / {0, 0} at the first push); SPNG_DONE with the final counts when last.
 * A capacity the stream outgrows: the push that overflows and every later one answer SPNG_E_OUTPUT_CAPACITY (written = the stream
 * bytes so far, beyond dst_cap; consumed and aux as for SPNG_NEED_MORE_INPUT: the pushes go on), the last one with written = the
 * bytes the whole stream needs and consumed = src_len; d_dst[0 .. dst_cap) = the stream's first dst_cap bytes.
 * Limit: the checksum sums of levels 0-7 (D1State.adlerS / adlerI, csrc/common.hpp) are 32-bit and grow by up to 65 520 per search
 * chunk and push: a stream of more than 65 536 chunks or pushes could wrap them. */
uint64_t spng_deflate_state_bytes(void);
int32_t spng_deflate_resume_batch(spng_ctx *ctx, const spng_stream_desc *descs, const int32_t *levels, void *const *d_states,
                                  const uint8_t *last, const uint64_t *h_state, uint32_t count,
                                  spng_result *d_results, spng_result *h_results);
/* replaces PNG.Encoder.pull end to end (PNG.Encoder.swift:33-129): storage -> zlib stream; d_rows is
 * scratch for the filtered scanlines (>= U bytes), d_idat receives the stream (capacity idat_len). */
int32_t spng_encode_batch(spng_ctx *ctx, const spng_image_desc *descs, int32_t level, uint32_t count,
                          spng_result *d_results, spng_result *h_results);

/* ---- several devices ------------------------------------------------------- */
/* Images are independent units: a batch is cut into contiguous blocks of ceil(count / parts) -- block `index` is
 * [*first, *first + *n) -- one per device (128 per GPU for 1024 images on 8). */
int32_t spng_shard(uint32_t count, uint32_t parts, uint32_t index, uint32_t *first, uint32_t *n);
/* spng_decode_batch (PNG.Context.push end to end) over n_ctx contexts, one per device of the node: descs[i]'s device
 * pointers live on the device of the context its block belongs to (spng_shard); every context decodes its block without
 * talking to the others.  d_gather (NULL: leave the rasters where they are): per image, where on the FIRST context's device its
 * raster is wanted -- the one exchange step of the path; each goes as a peer-to-peer copy on the context's own copy stream behind
 * the decode of its group (a shard goes in SPNG_CFG_MULTI_GROUPS groups, so a group's rasters travel while the next decodes;
 * xGMI is point to point: the seven peers' copies ride their own links at once).  Peer access to the first context's device is
 * switched on once per pair (hipDeviceCanAccessPeer / hipDeviceEnablePeerAccess); where the devices refuse, the copies are staged
 * by the runtime and spng_last_error_string says so.  The caller's current device is left as it was.  Returns when everything
 * has arrived; results in h_results. */
int32_t spng_decode_batch_multi(spng_ctx *const *ctxs, uint32_t n_ctx, const spng_image_desc *descs, uint32_t count,
                                void *const *d_gather, spng_result *h_results);

/* ---- measurement and housekeeping ------------------------------------------------------------------ */
/* The copy ceiling: milliseconds per copy of `bytes` from d_src to d_dst by a kernel of this library with nothing to do in
 * between (HIP events on the context's stream, `repeats` copies after a first touch).  pattern 0: 16 bytes per lane,
 * grid-stride -- the denominator next to the 8 TB/s spec peak.  pattern 1: 64 rows of 16384 bytes per wave in 256-byte tiles,
 * row r trailing row r - 1 by 4 bytes on both sides -- the access pattern of the scanline kernel before its stores were made
 * line-aligned: what that cost, and a known byte count in that pattern to calibrate FETCH_SIZE / WRITE_SIZE against. */
int32_t spng_copy_ceiling(spng_ctx *ctx, void *d_dst, const void *d_src, uint64_t bytes, int32_t pattern, int32_t repeats,
                          double *ms_per_copy);
/* Gives the context's scratch back to the device (token pool, symbol scratch, deflate slab and rings): the next call that
 * needs one allocates it again.  Waits for the context's work first. */
int32_t spng_trim(spng_ctx *ctx);
/* 1: this device's LDS serves the lanes of an atomic exchange on one address in ascending lane order (probed when the context was
 * created) and the deflater's match search inserts a batch of positions with ONE exchange per lane; 0: it keeps the read-back form.
 * No reference counterpart (which of two bit-identical code paths runs: bench and tests report it). */
int32_t spng_lds_exchange_ordered(spng_ctx *ctx, int32_t *ordered);

#ifdef __cplusplus
}
#endif
#endif
