// file_head.hpp -- the bytes of a PNG file between its signature and its first IDAT chunk, as PNG.Image.compress(stream:level:hint:)
// writes them (Sources/PNG/PNG.Image.swift:589-656): the reference's rules restated once, in plain C++17 without a HIP header, so that
// the host layer (host_files.hip) and a stand-alone test program (tools/file_head_main.cpp, built with g++ and with a sanitizer) run the
// very same code.  The order of the chunks:
//     CgBI                         PNG.Image.encode, PNG.Image.swift:416-423: [48, 0, 32, 6] for bgr8, [48, 0, 32, 2] for bgra8
//     IHDR                         PNG.Header.serialized, Parsing/PNG.Header.swift:133-145
//     the caller's blobs, group A  (cHRM gAMA sRGB iCCP sBIT in the reference, PNG.Image.swift:596-615)
//     PLTE  bKGD  tRNS             PNG.Layout.palette / .background / .transparency, Formats/PNG.Layout.swift:60-194, and the
//                                  `serialized` of PNG.Palette (:84-97), PNG.Background (:180-201), PNG.Transparency (:183-208)
//     the caller's blobs, group B  (hIST pHYs tIME iTXt sPLT and application chunks, PNG.Image.swift:630-656)
// The blobs are opaque: (type, bytes), framed and summed, neither interpreted nor reordered.  Lengths, types and CRC-32s are laid
// down here, on the host: they are small and host-known.
#ifndef SPNG_FILE_HEAD_HPP    // (not #pragma once: the header also compiles alone, as the main file)
#define SPNG_FILE_HEAD_HPP
#include <cstdint>
#include <cstring>
#include <vector>
#include "../../include/spng_mi355.h"

namespace spng {

// PNG.Chunk.init(validating:) (PNG.Chunk.swift:69-88): the rule of chunks.hip's valid_type, which spng_lex_batch applies
inline bool file_type_lexes(uint32_t name)
{
    switch (name) {
    case 0x43674249: case 0x49484452: case 0x504c5445: case 0x49444154: case 0x49454e44:   // CgBI IHDR PLTE IDAT IEND
    case 0x6348524d: case 0x67414d41: case 0x69434350: case 0x73424954: case 0x73524742:   // cHRM gAMA iCCP sBIT sRGB
    case 0x624b4744: case 0x68495354: case 0x74524e53: case 0x70485973: case 0x73504c54:   // bKGD hIST tRNS pHYs sPLT
    case 0x74494d45: case 0x69545874: case 0x74455874: case 0x7a545874:                     // tIME iTXt tEXt zTXt
        return true;
    default:
        return (name & 0x20002000u) == 0x20000000u;
    }
}
// the chunks the format itself writes: a blob may not be one of them
inline bool file_type_owned(uint32_t name)
{
    switch (name) {
    case 0x43674249: case 0x49484452: case 0x504c5445: case 0x624b4744: case 0x74524e53: case 0x49444154: case 0x49454e44:
        return true;                                           // CgBI IHDR PLTE bKGD tRNS IDAT IEND
    default:
        return false;
    }
}

// the standard reflected CRC-32 (polynomial 0xEDB88320), continued from a finished value
inline uint32_t file_crc32(uint32_t crc, const uint8_t *p, size_t n)
{
    static const struct Table {
        uint32_t v[256];
        Table() { for (uint32_t i = 0; i < 256; ++i) { uint32_t c = i; for (int k = 0; k < 8; ++k) c = c & 1 ? (c >> 1) ^ 0xedb88320u : c >> 1; v[i] = c; } }
    } table;
    crc ^= 0xffffffffu;
    for (size_t i = 0; i < n; ++i) crc = table.v[(crc ^ p[i]) & 0xff] ^ (crc >> 8);
    return crc ^ 0xffffffffu;
}

inline void file_put32(std::vector<uint8_t> &out, uint32_t v) { for (int k = 3; k >= 0; --k) out.push_back((uint8_t)(v >> (8 * k))); }
inline void file_put16(std::vector<uint8_t> &out, uint16_t v) { out.push_back((uint8_t)(v >> 8)); out.push_back((uint8_t)v); }

// PNG.BytestreamDestination.format(type:data:) (Lexing/PNG.BytestreamDestination.swift:66-88)
inline void file_put_chunk(std::vector<uint8_t> &out, uint32_t type, const uint8_t *data, size_t n)
{
    file_put32(out, (uint32_t)n);
    const size_t at = out.size();
    file_put32(out, type);
    if (n) out.insert(out.end(), data, data + n);
    file_put32(out, file_crc32(0, out.data() + at, n + 4));
}

enum class FileKind { v, va, rgb, rgba, indexed, none };
// the PNG.Format a desc names: v1 ... v16, va8 / va16, rgb8 / rgb16 / bgr8, rgba8 / rgba16 / bgra8, indexed1 ... indexed8
inline FileKind file_kind(const spng_png_desc &d)
{
    const bool sub = d.depth == 1 || d.depth == 2 || d.depth == 4, full = d.depth == 8 || d.depth == 16;
    if (d.indexed > 1 || d.bgr > 1 || d.interlaced > 1 || d.has_key > 1 || d.has_fill > 1 || d.reserved) return FileKind::none;
    if (d.indexed) return d.channels == 1 && !d.bgr && (sub || d.depth == 8) ? FileKind::indexed : FileKind::none;
    if (d.bgr) return d.depth != 8 ? FileKind::none : d.channels == 3 ? FileKind::rgb : d.channels == 4 ? FileKind::rgba : FileKind::none;
    if (d.channels == 1) return sub || full ? FileKind::v : FileKind::none;
    if (!full) return FileKind::none;
    return d.channels == 2 ? FileKind::va : d.channels == 3 ? FileKind::rgb : d.channels == 4 ? FileKind::rgba : FileKind::none;
}

// The head of the file `d` describes, appended to `out`: everything between the signature and the first IDAT.  -> SPNG_DONE, or
// SPNG_E_ARGUMENT (nothing appended) for what the writer refuses: a blob whose type the format owns or the lexer would not accept (or
// with bytes but no pointer), a palette count outside what the format allows, a width or height of 0, a depth / channels / flag
// combination that is no PNG.Format, a key where the format has none, a sample the format's field does not hold (PNG.Format.validate,
// Formats/PNG.Format.swift:274-351: the reference traps), chunk_bytes outside 1 ... 0x7fffffff.
inline int32_t file_head(const spng_png_desc &d, std::vector<uint8_t> &out)
{
    const FileKind kind = file_kind(d);
    if (kind == FileKind::none || !d.width || !d.height || !d.chunk_bytes || d.chunk_bytes > 0x7fffffffull) return SPNG_E_ARGUMENT;
    // palette cannot contain more entries than bit depth allows (PNG.Format.swift:276-309); the grey formats have none
    const uint32_t most = kind == FileKind::v || kind == FileKind::va ? 0u : 1u << (d.depth < 8 ? d.depth : 8);
    if (d.palette_count > most || (kind == FileKind::indexed && !d.palette_count) || (d.palette_count && !d.palette)) return SPNG_E_ARGUMENT;
    const bool keyed = kind == FileKind::v || kind == FileKind::rgb, wide = d.depth == 16;
    if (d.has_key && !keyed) return SPNG_E_ARGUMENT;
    const int fields = kind == FileKind::v || kind == FileKind::va ? 1 : kind == FileKind::indexed ? 1 : 3;
    for (int k = 0; k < fields; ++k) {
        // (8-bit keys and fills are UInt8 in the format; v1 / v2 / v4 fills above the depth's largest sample trap, :313-321)
        if (d.has_key && !wide && d.key[k] > 255) return SPNG_E_ARGUMENT;
        if (d.has_fill && kind != FileKind::indexed && !wide && d.fill[k] > 255) return SPNG_E_ARGUMENT;
        if (d.has_fill && kind == FileKind::v && d.depth < 8 && d.fill[k] >> d.depth) return SPNG_E_ARGUMENT;
    }
    if (d.has_fill && kind == FileKind::indexed && d.fill[0] >= d.palette_count) return SPNG_E_ARGUMENT;       // (:322-330)
    for (int g = 0; g < 2; ++g) {
        const spng_blob *blobs = g ? d.after : d.before;
        const uint32_t count = g ? d.after_count : d.before_count;
        if (count && !blobs) return SPNG_E_ARGUMENT;
        for (uint32_t i = 0; i < count; ++i)
            if (file_type_owned(blobs[i].type) || !file_type_lexes(blobs[i].type) || (blobs[i].len && !blobs[i].data) || blobs[i].len > 0x7fffffffu)
                return SPNG_E_ARGUMENT;
    }
    auto put_blobs = [&](const spng_blob *blobs, uint32_t count) {
        for (uint32_t i = 0; i < count; ++i) file_put_chunk(out, blobs[i].type, (const uint8_t *)blobs[i].data, blobs[i].len);
    };
    std::vector<uint8_t> data;
    if (d.bgr) {
        const uint8_t cgbi[4] = {48, 0, 32, (uint8_t)(d.channels == 3 ? 6 : 2)};
        file_put_chunk(out, 0x43674249, cgbi, 4);
    }
    // IHDR: PNG.Format.Pixel.code -- v: 0, rgb: 2, indexed: 3, va: 4, rgba: 6
    const uint8_t code = kind == FileKind::v ? 0 : kind == FileKind::rgb ? 2 : kind == FileKind::indexed ? 3 : kind == FileKind::va ? 4 : 6;
    file_put32(data, d.width); file_put32(data, d.height);
    data.push_back(d.depth); data.push_back(code); data.push_back(0); data.push_back(0); data.push_back(d.interlaced ? 1 : 0);
    file_put_chunk(out, 0x49484452, data.data(), data.size());
    put_blobs(d.before, d.before_count);
    // PLTE: every entry's (r, g, b); a colour format writes one only for a non-empty suggested palette (PNG.Layout.swift:60-90)
    if (d.palette_count) {
        data.clear();
        for (uint32_t i = 0; i < d.palette_count; ++i) data.insert(data.end(), d.palette + 4 * i, d.palette + 4 * i + 3);
        file_put_chunk(out, 0x504c5445, data.data(), data.size());
    }
    // bKGD (PNG.Layout.swift:141-194): a palette index, or 16-bit fields, 8-bit ones widened.  bgr8 / bgra8 hold (b, g, r); the layout
    // reads the fields by name, so the chunk is (r, g, b) again
    if (d.has_fill) {
        data.clear();
        if (kind == FileKind::indexed) data.push_back((uint8_t)d.fill[0]);
        else if (fields == 1) file_put16(data, d.fill[0]);
        else for (int k = 0; k < 3; ++k) file_put16(data, d.fill[d.bgr ? 2 - k : k]);
        file_put_chunk(out, 0x624b4744, data.data(), data.size());
    }
    // tRNS (PNG.Layout.swift:91-140): the key the same way; an indexed format the alphas up to the last one that is not 255, none
    // when all are
    if (kind == FileKind::indexed) {
        uint32_t upto = d.palette_count;
        while (upto && d.palette[4 * (upto - 1) + 3] == 255) --upto;
        if (upto) {
            data.clear();
            for (uint32_t i = 0; i < upto; ++i) data.push_back(d.palette[4 * i + 3]);
            file_put_chunk(out, 0x74524e53, data.data(), data.size());
        }
    } else if (d.has_key) {
        data.clear();
        if (fields == 1) file_put16(data, d.key[0]);
        else for (int k = 0; k < 3; ++k) file_put16(data, d.key[d.bgr ? 2 - k : k]);
        file_put_chunk(out, 0x74524e53, data.data(), data.size());
    }
    put_blobs(d.after, d.after_count);
    return SPNG_DONE;
}

// the exact size of the file for a stream of stream_len bytes (0: no such file, or a desc the writer refuses)
inline uint64_t file_bound(const spng_png_desc &d, uint64_t stream_len)
{
    std::vector<uint8_t> head;
    if (!stream_len || file_head(d, head) != SPNG_DONE) return 0;
    const uint64_t chunks = (stream_len + d.chunk_bytes - 1) / d.chunk_bytes;
    return 8 + head.size() + stream_len + 12 * chunks + 12;
}

}  // namespace spng

#endif
