// chunks.hip -- PNG chunk framing for gfx950: the callers' side of the decode / encode path.
//
// Replaces, for a batch of whole files resident in HBM:
//   signature + chunk lexing + CRC-32 check   Sources/PNG/Lexing/PNG.BytestreamSource.swift:44-108
//   chunk type validation                     Sources/PNG/Lexing/PNG.Chunk.swift:69-88
//   IHDR fields                               Sources/PNG/Parsing/PNG.Header.swift:73-129 (layout only)
//   the IDAT loop of decompress(stream:)      Sources/PNG/PNG.Image.swift:385-389 (payloads concatenated)
//   chunk emission + CRC-32                   Sources/PNG/Lexing/PNG.BytestreamDestination.swift:66-88
// CRC-32 is swift-hash 0.7.1's CRC32 (Package.resolved; source not in the reference checkout): the standard
// reflected CRC-32, polynomial 0xEDB88320, initial value and final xor 0xFFFFFFFF -- pinned by the two
// checksums in Sources/PNGIntegrationTests/ErrorHandling.swift:30,42 and by every fixture lexing cleanly.
//
// Three kernels.  `lex_walk_kernel`: one wave per file walks the chunk chain (a chunk's length field gives the next
// header: the only serial part), checks signature, types and bounds, notes IHDR / PLTE / tRNS and lists every chunk with
// the place its payload takes in the IDAT stream.  `lex_chunk_kernel`: one wave per listed chunk, all files at once:
// CRC-32 of type + data against the declared one (wave-parallel: 64 pieces of 16-byte loads, slicing-by-4, folded in
// GF(2)[x] / P, crc32.hpp) and the IDAT payload copied into place with 16-byte moves.  `lex_finish_kernel`: the first
// thing that went wrong in FILE ORDER decides the result, as in the reference's loop (a bad checksum in chunk 3 hides a
// bad type in chunk 5).  A file with more chunks than its list holds is walked on by its own wave the serial way.
#include "common.hpp"
#include "crc32.hpp"
#include "geometry.hpp"

namespace spng {

__device__ __forceinline__ uint32_t be32(const gbyte *p) { return (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | p[3]; }

// PNG.Chunk.init(validating:) (PNG.Chunk.swift:69-88)
__device__ __forceinline__ bool valid_type(uint32_t name)
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

// a listed chunk
struct LexChunk { uint64_t off, idat_off; uint32_t length, name; uint32_t declared, computed; };
// what the walk leaves for the finish
struct LexWalk { uint32_t listed, stop_index; int32_t stop_status; uint32_t pad; uint64_t stop_aux, stop_off, stop_idat; uint32_t bad_crc, ihdr_at, plte_at, trns_at, cgbi_at, pad2; };

__device__ __forceinline__ void copy_bytes(gbyte *dst, const gbyte *src, uint64_t n, int lane)
{
    typedef uint32_t c4 __attribute__((vector_size(16)));
    struct __attribute__((packed)) P16 { c4 v; };
    typedef P16 __attribute__((address_space(1))) gP16;
    const uint64_t units = n / 16;
    for (uint64_t u = lane; u < units; u += 64) ((gP16 *)(dst + u * 16))->v = ((const gP16 *)(src + u * 16))->v;
    for (uint64_t i = units * 16 + lane; i < n; i += 64) dst[i] = src[i];
}

// CRC-32 over a chunk's type code and data (BytestreamSource.chunk, :95-103; BytestreamDestination.format, :75-83)
__device__ __forceinline__ uint32_t chunk_crc32(const uint32_t *tab, uint32_t name, const gbyte *data, uint64_t length, int lane)
{
    uint32_t c = 0xffffffffu;
    for (int b = 0; b < 4; ++b) c = tab[(c ^ (name >> (8 * (3 - b)))) & 0xff] ^ (c >> 8);
    return wave_crc32(tab, data, length, c ^ 0xffffffffu, lane);
}

__global__ __launch_bounds__(64) void lex_walk_kernel(const spng_file_desc *__restrict__ files, spng_lexed *__restrict__ out,
                                                      LexChunk *__restrict__ table, const uint64_t *__restrict__ table_at,
                                                      LexWalk *__restrict__ walks)
{
    __shared__ uint32_t tab[CRC_TAB];
    const int lane = threadIdx.x;
    const spng_file_desc f = files[blockIdx.x];
    const gbyte *p = (const gbyte *)uni64((uint64_t)f.d_png);
    const uint64_t n = uni64(f.len);
    gbyte *idat = (gbyte *)uni64((uint64_t)f.d_idat);
    const uint64_t cap = uni64(f.idat_cap);
    LexChunk *list = table + uni64(table_at[blockIdx.x]);
    const uint32_t list_cap = (uint32_t)(uni64(table_at[blockIdx.x + 1]) - uni64(table_at[blockIdx.x]));
    spng_lexed r;
    memset(&r, 0, sizeof r);
    LexWalk w;
    memset(&w, 0, sizeof w);
    w.stop_status = SPNG_DONE; w.bad_crc = 0xffffffffu;
    w.ihdr_at = w.plte_at = w.trns_at = w.cgbi_at = 0xffffffffu;
    uint64_t off = 8, idat_len = 0;
    uint32_t index = 0;
    bool tabled = false;
    // signature() (:44-56)
    if (n < 8) w.stop_status = SPNG_E_TRUNCATED_SIGNATURE;
    else {
        const uint64_t sig = (uint64_t)be32(p) << 32 | be32(p + 4);
        if (sig != 0x89504e470d0a1a0aull) { w.stop_status = SPNG_E_SIGNATURE; w.stop_aux = sig; }
    }
    while (w.stop_status == SPNG_DONE) {
        // chunk() (:71-108)
        if (off + 8 > n) { w.stop_status = SPNG_E_TRUNCATED_CHUNK_HEADER; break; }
        const uint32_t length = be32(p + off), name = be32(p + off + 4);
        if (!valid_type(name)) { w.stop_status = SPNG_E_CHUNK_TYPE; w.stop_aux = name; break; }
        const uint64_t bytes = (uint64_t)length + 4;
        if (off + 8 + bytes > n) { w.stop_status = SPNG_E_TRUNCATED_CHUNK_BODY; w.stop_aux = bytes; break; }
        const gbyte *data = p + off + 8;
        if (name == 0x49444154 && idat_len + length > cap) {
            // (the reference's order: the checksum first)
            if (!tabled) { crc_table(tab, lane); tabled = true; }
            const uint32_t declared = be32(data + length), computed = wave_crc32(tab, p + off + 4, (uint64_t)length + 4, 0, lane);
            if (declared != computed) { w.stop_status = SPNG_E_CHUNK_CHECKSUM; w.stop_aux = (uint64_t)declared << 32 | computed; }
            else w.stop_status = SPNG_E_OUTPUT_CAPACITY;
            break;
        }
        if (index < list_cap) {
            if (lane == 0) {
                LexChunk c;
                c.off = off; c.idat_off = idat_len; c.length = length; c.name = name; c.declared = be32(data + length); c.computed = 0;
                list[index] = c;
            }
        } else {
            // the list is full: this wave checks and copies the rest itself
            if (!tabled) { crc_table(tab, lane); tabled = true; }
            const uint32_t declared = be32(data + length);
            const uint32_t computed = wave_crc32(tab, p + off + 4, (uint64_t)length + 4, 0, lane);
            if (declared != computed) { w.stop_status = SPNG_E_CHUNK_CHECKSUM; w.stop_aux = (uint64_t)declared << 32 | computed; break; }
            if (name == 0x49444154) copy_bytes(idat + idat_len, data, length, lane);
        }
        if (name == 0x43674249) w.cgbi_at = w.cgbi_at == 0xffffffffu ? index : w.cgbi_at;
        else if (name == 0x49484452 && length >= 13) {
            r.width = be32(data); r.height = be32(data + 4);
            r.depth = data[8]; r.color = data[9]; r.compression = data[10]; r.filter = data[11]; r.interlace = data[12];
            w.ihdr_at = index;
        } else if (name == 0x504c5445) { r.plte_off = off + 8; r.plte_len = length; w.plte_at = index; }
        else if (name == 0x74524e53) { r.trns_off = off + 8; r.trns_len = length; w.trns_at = index; }
        else if (name == 0x49444154) idat_len += length;
        index += 1;
        off += 8 + bytes;
        if (name == 0x49454e44) break;                         // IEND
    }
    w.listed = index < list_cap ? index : list_cap;
    w.stop_index = index; w.stop_off = off; w.stop_idat = idat_len;
    if (lane == 0) { out[blockIdx.x] = r; walks[blockIdx.x] = w; }
}

__global__ __launch_bounds__(64) void lex_chunk_kernel(const spng_file_desc *__restrict__ files, LexChunk *__restrict__ table,
                                                       const uint64_t *__restrict__ table_at, LexWalk *__restrict__ walks)
{
    __shared__ uint32_t tab[CRC_TAB];
    const int lane = threadIdx.x;
    const uint32_t file = blockIdx.y;
    const uint32_t listed = UNI(walks[file].listed);
    if (blockIdx.x >= listed) return;
    const spng_file_desc f = files[file];
    const gbyte *p = (const gbyte *)uni64((uint64_t)f.d_png);
    gbyte *idat = (gbyte *)uni64((uint64_t)f.d_idat);
    LexChunk *list = table + uni64(table_at[file]);
    crc_table(tab, lane);
    for (uint32_t k = blockIdx.x; k < listed; k += gridDim.x) {
        const uint64_t off = uni64(list[k].off);
        const uint32_t length = UNI(list[k].length), name = UNI(list[k].name), declared = UNI(list[k].declared);
        // (the copy stays a pass of its own: consecutive lanes, consecutive 16-byte units.  Copied by the lanes that sum them -- a
        // piece per lane, 2^k bytes apart -- the payloads of 64 KiB chunks cost a line per lane and store: 256 4K files lexed in 10.0
        // instead of 6.9 ms)
        const uint32_t computed = chunk_crc32(tab, name, p + off + 8, length, lane);
        if (declared != computed) {
            if (lane == 0) { list[k].computed = computed; atomicMin(&walks[file].bad_crc, k); }
        } else if (name == 0x49444154) copy_bytes(idat + uni64(list[k].idat_off), p + off + 8, length, lane);
    }
}

__global__ void lex_finish_kernel(spng_lexed *__restrict__ out, const LexChunk *__restrict__ table, const uint64_t *__restrict__ table_at,
                                  const LexWalk *__restrict__ walks, const spng_file_desc *__restrict__ files, uint32_t count)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    spng_lexed r = out[i];
    const LexWalk w = walks[i];
    const LexChunk *list = table + table_at[i];
    uint32_t upto = w.stop_index;                              // chunks lexed in full
    r.status = w.stop_status;
    if (w.stop_status == SPNG_E_CHUNK_CHECKSUM) { r.aux[0] = w.stop_aux >> 32; r.aux[1] = (uint32_t)w.stop_aux; }
    else r.aux[0] = w.stop_aux;
    r.consumed = w.stop_off; r.idat_len = w.stop_idat;
    if (w.bad_crc < upto) {
        // a checksum failed in front of whatever stopped the walk
        const LexChunk c = list[w.bad_crc];
        upto = w.bad_crc;
        r.status = SPNG_E_CHUNK_CHECKSUM; r.aux[0] = c.declared; r.aux[1] = c.computed;
        r.consumed = c.off; r.idat_len = c.idat_off;
    }
    r.chunks = upto;
    // what lies behind the first failure was never seen by the reference's loop
    if (w.ihdr_at >= upto) { r.width = r.height = 0; r.depth = r.color = r.compression = r.filter = r.interlace = 0; }
    if (w.plte_at >= upto) { r.plte_off = 0; r.plte_len = 0; }
    if (w.trns_at >= upto) { r.trns_off = 0; r.trns_len = 0; }
    r.ios = w.cgbi_at < upto ? 1 : 0;
    if (r.consumed > files[i].len) r.consumed = files[i].len;
    out[i] = r;
}

// ---- the chunk directory (spng_lex_dir_batch) -------------------------------------------------------------------------------
// Behind the three kernels above, which it leaves as they are: `dir_list_kernel`, a wave per file, writes an entry per chunk lexed
// in full (lex_finish_kernel's `chunks`) -- the listed ones from the list, a lane each; the ones the walking wave handled itself once
// the list was full by walking their headers again from the last listed chunk on (every one of them has been checked against the
// file's length by the walk).  `dir_head_kernel`, a wave per entry, parses the heads of tEXt / zTXt / iTXt / iCCP:
//   PNG.Text.init(parsing:unicode:)     Sources/PNG/Parsing/PNG.Text.swift:110-200
//   name(parsing:), validate(name:)     :202-251       language(parsing:), validate(language:)    :254-301
//   PNG.ColorProfile.init(parsing:)     Sources/PNG/Parsing/PNG.ColorProfile.swift:51-85  (up to the inflator)
// The separators are found 64 bytes at a time: a byte per lane, a ballot, the first set bit.
static constexpr uint32_t T_tEXt = 0x74455874, T_zTXt = 0x7a545874, T_iTXt = 0x69545874, T_iCCP = 0x69434350;

// the first NUL of payload[from, to), or SPNG_NO_OFFSET
__device__ __forceinline__ uint32_t find_nul(const gbyte *payload, uint32_t from, uint32_t to, int lane)
{
    for (uint64_t base = from; base < to; base += 64) {
        const uint64_t i = base + lane;
        const unsigned long long hit = __ballot(i < to && payload[i] == 0);
        if (hit) return (uint32_t)base + (uint32_t)__ffsll((long long)hit) - 1;
    }
    return SPNG_NO_OFFSET;
}

// validate(name:) over payload[0, k) (:226-251): 1 ... 80 scalars of 0x20 ... 0x7d or 0xa1 ... 0xff, no leading, trailing or doubled space
__device__ __forceinline__ bool valid_keyword(const gbyte *payload, uint32_t k, int lane)
{
    if (k < 1 || k > 80) return false;
    bool bad = false;
    for (uint32_t i = lane; i < k; i += 64) {
        const uint32_t c = payload[i], prev = payload[i ? i - 1 : 0];
        bad = bad || !((c >= 0x20 && c <= 0x7d) || c >= 0xa1) || (prev == 0x20 && c == 0x20) || (i == k - 1 && c == 0x20);
    }
    return __ballot(bad) == 0;
}

// language(parsing:) over payload[from, l), l > from (:254-301): subtags between '-' of 1 ... 8 letters each.  -> the payload offset of
// the first subtag that is none, or SPNG_NO_OFFSET.  The start of the subtag a position lies in never decreases along the tag, so the
// first position that breaks a rule names the first bad subtag.
__device__ __forceinline__ uint32_t bad_subtag(const gbyte *payload, uint32_t from, uint32_t l, int lane)
{
    uint32_t start = from;                                     // of the subtag in progress where the 64 bytes begin
    for (uint64_t base = from; base <= l; base += 64) {
        const uint64_t i = base + lane;
        const uint32_t c = i < l ? payload[i] : 0x2d;          // (the NUL ends the last subtag as a '-' ends the others)
        const bool in = i <= l, dash = in && c == 0x2d;
        const unsigned long long dashes = __ballot(dash), below = dashes & ((1ull << lane) - 1);
        const uint32_t mine = below ? (uint32_t)base + 64 - (uint32_t)__clzll((long long)below) : start;
        const bool letter = (c | 0x20) >= 0x61 && (c | 0x20) <= 0x7a;
        const bool fails = in && (dash ? (uint32_t)i == mine : !letter || (uint32_t)i - mine >= 8);
        const unsigned long long failed = __ballot(fails);
        if (failed) return (uint32_t)__shfl((int)mine, __ffsll((long long)failed) - 1);
        if (dashes) start = (uint32_t)base + 64 - (uint32_t)__clzll((long long)dashes);
    }
    return SPNG_NO_OFFSET;
}

struct Head { int32_t status; uint32_t aux, k, l, m, body_off, compressed; };
__device__ __forceinline__ Head parse_head(uint32_t name, const gbyte *payload, uint32_t length, int lane)
{
    Head h;
    h.status = SPNG_DONE; h.aux = 0; h.k = h.l = h.m = SPNG_NO_OFFSET; h.body_off = 0; h.compressed = 0;
    const bool profile = name == T_iCCP;
    const uint32_t k = find_nul(payload, 0, length, lane);
    if (k != SPNG_NO_OFFSET) h.k = k;
    if (k == SPNG_NO_OFFSET || !valid_keyword(payload, k, lane)) {
        h.status = profile ? SPNG_E_PROFILE_NAME : SPNG_E_TEXT_KEYWORD; h.aux = k != SPNG_NO_OFFSET;
        return h;
    }
    if (profile) {
        if ((uint64_t)k + 1 >= length) { h.status = SPNG_E_PROFILE_CHUNK_LENGTH; h.aux = k + 2; return h; }
        if (payload[k + 1] != 0) { h.status = SPNG_E_PROFILE_COMPRESSION_METHOD; h.aux = payload[k + 1]; return h; }
        h.compressed = 1; h.body_off = k + 2;
        return h;
    }
    if (name != T_iTXt) {
        // the one Latin-1 path of tEXt and zTXt: a second NUL means compressed (:181)
        h.compressed = (uint64_t)k + 1 < length && payload[k + 1] == 0;
        h.body_off = k + 1 + h.compressed;
        return h;
    }
    if ((uint64_t)k + 2 >= length) { h.status = SPNG_E_TEXT_CHUNK_LENGTH; h.aux = k + 3; return h; }
    const uint32_t l = find_nul(payload, k + 3, length, lane);
    if (l == SPNG_NO_OFFSET) { h.status = SPNG_E_TEXT_LANGUAGE; return h; }
    h.l = l;
    if (l > k + 3) {
        const uint32_t bad = bad_subtag(payload, k + 3, l, lane);
        if (bad != SPNG_NO_OFFSET) { h.status = SPNG_E_TEXT_LANGUAGE; h.aux = 1 + bad; return h; }
    }
    const uint32_t m = find_nul(payload, l + 1, length, lane);
    if (m == SPNG_NO_OFFSET) { h.status = SPNG_E_TEXT_LOCALIZED_KEYWORD; return h; }
    h.m = m;
    const uint32_t flag = payload[k + 1], method = payload[k + 2];
    if (flag == 1 && method != 0) { h.status = SPNG_E_TEXT_COMPRESSION_METHOD; h.aux = method; return h; }
    if (flag > 1) { h.status = SPNG_E_TEXT_COMPRESSION; h.aux = flag; return h; }
    h.compressed = flag; h.body_off = m + 1;
    return h;
}

__global__ __launch_bounds__(64) void dir_list_kernel(const spng_file_desc *__restrict__ files, const spng_chunk_dir *__restrict__ dirs,
                                                      const spng_lexed *__restrict__ out, const LexChunk *__restrict__ table,
                                                      const uint64_t *__restrict__ table_at, const LexWalk *__restrict__ walks)
{
    const int lane = threadIdx.x;
    const uint32_t file = blockIdx.x;
    const uint32_t chunks = UNI(out[file].chunks), cap = UNI(dirs[file].cap);
    const uint32_t n = chunks < cap ? chunks : cap, listed = UNI(walks[file].listed);
    spng_chunk_entry *entries = (spng_chunk_entry *)uni64((uint64_t)dirs[file].d_entries);
    const LexChunk *list = table + uni64(table_at[file]);
    spng_chunk_entry e;
    memset(&e, 0, sizeof e);
    e.status = SPNG_DONE; e.k = e.l = e.m = SPNG_NO_OFFSET;
    const uint32_t from_list = n < listed ? n : listed;
    for (uint32_t i = lane; i < from_list; i += 64) {
        e.type = list[i].name; e.length = list[i].length; e.offset = list[i].off + 8;
        entries[i] = e;
    }
    if (n <= listed) return;
    // the list was full: the headers behind it once more, the serial way
    const gbyte *p = (const gbyte *)uni64((uint64_t)files[file].d_png);
    uint64_t off = listed ? uni64(list[listed - 1].off) + 12 + UNI(list[listed - 1].length) : 8;
    for (uint32_t i = listed; i < n; ++i) {
        e.length = be32(p + off); e.type = be32(p + off + 4); e.offset = off + 8;
        if (lane == 0) entries[i] = e;
        off += 12 + (uint64_t)e.length;
    }
}

__global__ __launch_bounds__(64) void dir_head_kernel(const spng_file_desc *__restrict__ files, const spng_chunk_dir *__restrict__ dirs,
                                                      const spng_lexed *__restrict__ out)
{
    const int lane = threadIdx.x;
    const uint32_t file = blockIdx.y;
    const uint32_t chunks = UNI(out[file].chunks), cap = UNI(dirs[file].cap);
    const uint32_t n = chunks < cap ? chunks : cap;
    spng_chunk_entry *entries = (spng_chunk_entry *)uni64((uint64_t)dirs[file].d_entries);
    const gbyte *p = (const gbyte *)uni64((uint64_t)files[file].d_png);
    for (uint32_t i = blockIdx.x; i < n; i += gridDim.x) {
        const uint32_t name = UNI(entries[i].type), length = UNI(entries[i].length);
        if (name != T_tEXt && name != T_zTXt && name != T_iTXt && name != T_iCCP) continue;
        const Head h = parse_head(name, p + uni64(entries[i].offset), length, lane);
        if (lane == 0) {
            spng_chunk_entry &e = entries[i];
            e.status = h.status; e.aux = h.aux; e.k = h.k; e.l = h.l; e.m = h.m; e.body_off = h.body_off; e.compressed = (uint8_t)h.compressed;
        }
    }
}

// ---- the typed chunks (spng_parse_dir_batch) --------------------------------------------------------------------------------
// Behind the directory, over what it left on the device: a record per entry with the answer of the reference's parser for that chunk,
//   PNG.Header.init(parsing:standard:)         Sources/PNG/Parsing/PNG.Header.swift:73-129
//   PNG.Palette.init(parsing:pixel:)           PNG.Palette.swift:54-81          PNG.Histogram.init(parsing:palette:)    PNG.Histogram.swift:49-61
//   PNG.Transparency.init(parsing:...)         PNG.Transparency.swift:126-180   PNG.Background.init(parsing:...)        PNG.Background.swift:119-176
//   PNG.SignificantBits.init(parsing:pixel:)   PNG.SignificantBits.swift:60-110 PNG.SuggestedPalette.init(parsing:)     PNG.SuggestedPalette.swift:54-156
//   PNG.Gamma, Chromaticity, ColorRendering, PhysicalDimensions, TimeModified .init(parsing:)
// its checks in its order.  `parse_scope_kernel`, a wave per file: the header -- entry 0, or entry 1 behind CgBI -- and the first PLTE
// among the entries (64 types per step, a ballot, the first set bit), parsed against the header: what every other parser of the file
// is handed (PNG.Image.swift:298-400, PNG.Metadata.swift:151-246).  `parse_value_kernel`, a wave per entry on dir_head_kernel's grid:
// a wave-uniform branch per chunk type; the first 64 bytes of the payload a byte per lane, fields read across the lanes; the
// frequencies of an sPLT 64 entries per step, each lane's against its left neighbour's.  `parse_first_kernel`, a wave per file: the
// first record in file order that holds an error -- read from the records once they are all there, so no order in which the waves
// finish can change it.
static constexpr uint32_t T_CgBI = 0x43674249, T_IHDR = 0x49484452, T_PLTE = 0x504c5445, T_tRNS = 0x74524e53, T_bKGD = 0x624b4744,
                          T_hIST = 0x68495354, T_gAMA = 0x67414d41, T_cHRM = 0x6348524d, T_sRGB = 0x73524742, T_sBIT = 0x73424954,
                          T_pHYs = 0x70485973, T_tIME = 0x74494d45, T_sPLT = 0x73504c54;

// what a file's parsers are handed: the pixel format (depth 0: no header), the standard, the entries of the palette in front of the chunk
struct ParseScope { uint32_t depth, color, ios; bool palette; uint32_t palette_count; };

__device__ __forceinline__ bool parsed_type(uint32_t name)
{
    return name == T_IHDR || name == T_PLTE || name == T_tRNS || name == T_bKGD || name == T_hIST || name == T_gAMA || name == T_cHRM ||
           name == T_sRGB || name == T_sBIT || name == T_pHYs || name == T_tIME || name == T_sPLT;
}
// PNG.Format.Pixel.recognize(code:) (Formats/PNG.Format.swift)
__device__ __forceinline__ bool pixel_format(uint32_t depth, uint32_t color)
{
    switch (color) {
    case 0: return depth == 1 || depth == 2 || depth == 4 || depth == 8 || depth == 16;
    case 3: return depth == 1 || depth == 2 || depth == 4 || depth == 8;
    case 2: case 4: case 6: return depth == 8 || depth == 16;
    default: return false;
    }
}
// byte j of the payload's first 64, which the lanes hold a byte each; big-endian fields from there
__device__ __forceinline__ uint32_t at8(uint32_t b, int j) { return (uint32_t)__shfl((int)b, j); }
__device__ __forceinline__ uint32_t at16(uint32_t b, int j) { return at8(b, j) << 8 | at8(b, j + 1); }
__device__ __forceinline__ uint32_t at32(uint32_t b, int j) { return at16(b, j) << 16 | at16(b, j + 2); }

__device__ __forceinline__ spng_chunk_value parse_fail(spng_chunk_value r, int32_t status, uint64_t aux0, uint64_t aux1 = 0)
{
    r.status = status; r.aux[0] = aux0; r.aux[1] = aux1;
    return r;
}

// descendingFrequency (PNG.SuggestedPalette.swift:125-156) over `entries` of `stride` bytes: -> the index of the first entry whose
// frequency -- its last two bytes -- exceeds its predecessor's (the first one's: UInt16.max), or SPNG_NO_OFFSET
__device__ __forceinline__ uint32_t first_ascent(const gbyte *data, uint32_t entries, uint32_t stride, int lane)
{
    uint32_t carry = 0xffff;                                   // the frequency in front of the step
    for (uint64_t base = 0; base < entries; base += 64) {
        const uint64_t i = base + lane;
        const bool in = i < entries;
        const uint32_t cur = in ? (uint32_t)data[i * stride + stride - 2] << 8 | data[i * stride + stride - 1] : 0;
        uint32_t prev = (uint32_t)__shfl_up((int)cur, 1);
        if (lane == 0) prev = carry;
        const unsigned long long up = __ballot(in && cur > prev);
        if (up) return (uint32_t)base + (uint32_t)__ffsll((long long)up) - 1;
        carry = (uint32_t)__shfl((int)cur, 63);
    }
    return SPNG_NO_OFFSET;
}

// one chunk.  Every argument but `lane` is the same in all lanes, and so is every branch
__device__ __forceinline__ spng_chunk_value parse_value(uint32_t name, const gbyte *payload, uint32_t length, const ParseScope s, int lane)
{
    spng_chunk_value r;
    memset(&r, 0, sizeof r);
    r.status = SPNG_DONE; r.scope = SPNG_SCOPE_NONE; r.k = SPNG_NO_OFFSET;
    if (!parsed_type(name)) return r;
    if (!s.depth) { r.scope = SPNG_SCOPE_NO_HEADER; return r; }
    const bool indexed = s.color == 3, has_color = (s.color & 2) != 0, has_alpha = (s.color & 4) != 0;
    if ((name == T_hIST || ((name == T_tRNS || name == T_bKGD) && indexed)) && !s.palette) { r.scope = SPNG_SCOPE_NO_PALETTE; return r; }
    r.scope = SPNG_SCOPE_PARSED;
    const uint32_t b = (uint32_t)lane < length ? payload[lane] : 0;
    const uint32_t sample_max = 0xffffu >> (16 - s.depth);
    if (name == T_IHDR) {
        if (length != 13) return parse_fail(r, SPNG_E_PARSE_HEADER_CHUNK_LENGTH, length);
        const uint32_t depth = at8(b, 8), color = at8(b, 9), compression = at8(b, 10), filter = at8(b, 11), interlace = at8(b, 12);
        if (!pixel_format(depth, color)) return parse_fail(r, SPNG_E_PARSE_HEADER_PIXEL_FORMAT_CODE, depth, color);
        if (s.ios && !(depth == 8 && (color == 2 || color == 6))) return parse_fail(r, SPNG_E_PARSE_HEADER_PIXEL_FORMAT, depth, color);
        if (compression) return parse_fail(r, SPNG_E_PARSE_HEADER_COMPRESSION_METHOD, compression);
        if (filter) return parse_fail(r, SPNG_E_PARSE_HEADER_FILTER, filter);
        if (interlace > 1) return parse_fail(r, SPNG_E_PARSE_HEADER_INTERLACING, interlace);
        const uint32_t x = at32(b, 0), y = at32(b, 4);
        if (!x || !y) return parse_fail(r, SPNG_E_PARSE_HEADER_SIZE, x, y);
        r.v[0] = x; r.v[1] = y; r.v[2] = depth; r.v[3] = color; r.v[4] = interlace;
    } else if (name == T_PLTE) {
        if (!has_color) return parse_fail(r, SPNG_E_PARSE_UNEXPECTED_PALETTE, s.depth, s.color);
        if (length % 3) return parse_fail(r, SPNG_E_PARSE_PALETTE_CHUNK_LENGTH, length);
        const uint32_t count = length / 3, most = 1u << (s.depth < 8 ? s.depth : 8);
        if (count < 1 || count > most) return parse_fail(r, SPNG_E_PARSE_PALETTE_COUNT, count, most);
        r.count = count;
    } else if (name == T_tRNS || name == T_bKGD) {
        const bool fill = name == T_bKGD;
        if (has_alpha && !fill) return parse_fail(r, SPNG_E_PARSE_UNEXPECTED_TRANSPARENCY, s.depth, s.color);
        if (indexed && !fill) {
            if (length > s.palette_count) return parse_fail(r, SPNG_E_PARSE_TRANSPARENCY_COUNT, length, s.palette_count);
            r.count = length;
        } else if (indexed) {
            if (length != 1) return parse_fail(r, SPNG_E_PARSE_BACKGROUND_CHUNK_LENGTH, length, 1);
            const uint32_t index = at8(b, 0);
            if (index >= s.palette_count) return parse_fail(r, SPNG_E_PARSE_BACKGROUND_INDEX, index, s.palette_count - 1);
            r.v[0] = index;
        } else {
            const uint32_t samples = has_color ? 3 : 1;
            if (length != 2 * samples)
                return parse_fail(r, fill ? SPNG_E_PARSE_BACKGROUND_CHUNK_LENGTH : SPNG_E_PARSE_TRANSPARENCY_CHUNK_LENGTH, length, 2 * samples);
            const uint32_t c0 = at16(b, 0), c1 = at16(b, 2), c2 = at16(b, 4);      // (behind a grey sample: zeros)
            const uint32_t top = c0 > c1 ? (c0 > c2 ? c0 : c2) : (c1 > c2 ? c1 : c2);
            if (top > sample_max) return parse_fail(r, fill ? SPNG_E_PARSE_BACKGROUND_SAMPLE : SPNG_E_PARSE_TRANSPARENCY_SAMPLE, top, sample_max);
            r.v[0] = c0; r.v[1] = c1; r.v[2] = c2;
        }
    } else if (name == T_hIST) {
        if (length != 2 * s.palette_count) return parse_fail(r, SPNG_E_PARSE_HISTOGRAM_CHUNK_LENGTH, length, 2 * s.palette_count);
        r.count = length / 2;
    } else if (name == T_gAMA) {
        if (length != 4) return parse_fail(r, SPNG_E_PARSE_GAMMA_CHUNK_LENGTH, length);
        r.v[0] = at32(b, 0);
    } else if (name == T_cHRM) {
        if (length != 32) return parse_fail(r, SPNG_E_PARSE_CHROMATICITY_CHUNK_LENGTH, length);
        for (int j = 0; j < 8; ++j) r.v[j] = at32(b, 4 * j);
    } else if (name == T_sRGB) {
        if (length != 1) return parse_fail(r, SPNG_E_PARSE_RENDERING_CHUNK_LENGTH, length);
        const uint32_t code = at8(b, 0);
        if (code > 3) return parse_fail(r, SPNG_E_PARSE_RENDERING_CODE, code);
        r.v[0] = code;
    } else if (name == T_sBIT) {
        const uint32_t arity = (has_color ? 3 : 1) + (has_alpha ? 1 : 0), most = indexed ? 8 : s.depth;
        if (length != arity) return parse_fail(r, SPNG_E_PARSE_SIGNIFICANT_BITS_CHUNK_LENGTH, length, arity);
        const unsigned long long bad = __ballot((uint32_t)lane < arity && (b < 1 || b > most));
        if (bad) return parse_fail(r, SPNG_E_PARSE_SIGNIFICANT_BITS_PRECISION, at8(b, __ffsll((long long)bad) - 1), most);
        for (int j = 0; j < 4; ++j) r.v[j] = at8(b, j);
    } else if (name == T_pHYs) {
        if (length != 9) return parse_fail(r, SPNG_E_PARSE_PHYSICAL_CHUNK_LENGTH, length);
        const uint32_t unit = at8(b, 8);
        if (unit > 1) return parse_fail(r, SPNG_E_PARSE_PHYSICAL_UNIT, unit);
        r.v[0] = at32(b, 0); r.v[1] = at32(b, 4); r.v[2] = unit;
    } else if (name == T_tIME) {
        if (length != 7) return parse_fail(r, SPNG_E_PARSE_TIME_CHUNK_LENGTH, length);
        // month, day, hour, minute, second in lanes 2 ... 6: each against its own range
        const uint32_t lo = lane == 2 || lane == 3 ? 1 : 0, hi = lane == 2 ? 12 : lane == 3 ? 31 : lane == 4 ? 23 : lane == 5 ? 59 : 60;
        const unsigned long long bad = __ballot(lane >= 2 && lane <= 6 && (b < lo || b > hi));
        const uint32_t year = at16(b, 0), month = at8(b, 2), day = at8(b, 3), hour = at8(b, 4), minute = at8(b, 5), second = at8(b, 6);
        if (bad) return parse_fail(r, SPNG_E_PARSE_TIME, year | month << 16 | day << 24, hour | minute << 8 | second << 16);
        r.v[0] = year; r.v[1] = month; r.v[2] = day; r.v[3] = hour; r.v[4] = minute; r.v[5] = second;
    } else {                                                   // sPLT
        const uint32_t k = find_nul(payload, 0, length, lane);
        if (k != SPNG_NO_OFFSET) r.k = k;
        if (k == SPNG_NO_OFFSET || !valid_keyword(payload, k, lane)) return parse_fail(r, SPNG_E_PARSE_SUGGESTED_PALETTE_NAME, k != SPNG_NO_OFFSET);
        if ((uint64_t)k + 1 >= length) return parse_fail(r, SPNG_E_PARSE_SUGGESTED_PALETTE_CHUNK_LENGTH, length, (uint64_t)k + 2);
        const uint32_t bytes = length - k - 2, code = payload[k + 1];
        if (code != 8 && code != 16) return parse_fail(r, SPNG_E_PARSE_SUGGESTED_PALETTE_DEPTH, code);
        const uint32_t stride = code == 8 ? 6 : 10;
        if (bytes % stride) return parse_fail(r, SPNG_E_PARSE_SUGGESTED_PALETTE_DATA_LENGTH, bytes, stride);
        const uint32_t up = first_ascent(payload + k + 2, bytes / stride, stride, lane);
        if (up != SPNG_NO_OFFSET) return parse_fail(r, SPNG_E_PARSE_SUGGESTED_PALETTE_FREQUENCY, up);
        r.count = bytes / stride; r.v[0] = code;
    }
    return r;
}

__global__ __launch_bounds__(64) void parse_scope_kernel(const spng_file_desc *__restrict__ files, const spng_chunk_dir *__restrict__ dirs,
                                                         const spng_lexed *__restrict__ out, spng_chunk_value *const *__restrict__ values,
                                                         spng_parsed *__restrict__ parsed)
{
    const int lane = threadIdx.x;
    const uint32_t file = blockIdx.x;
    const uint32_t chunks = UNI(out[file].chunks), cap = UNI(dirs[file].cap);
    const uint32_t n = chunks < cap ? chunks : cap;
    const spng_chunk_entry *entries = (const spng_chunk_entry *)uni64((uint64_t)dirs[file].d_entries);
    spng_chunk_value *vals = (spng_chunk_value *)uni64((uint64_t)values[file]);
    const gbyte *p = (const gbyte *)uni64((uint64_t)files[file].d_png);
    spng_parsed r;
    memset(&r, 0, sizeof r);
    r.status = SPNG_DONE; r.index = r.ihdr_index = r.plte_index = SPNG_NO_OFFSET;
    ParseScope s;
    s.depth = s.color = s.ios = s.palette_count = 0; s.palette = false;
    // PNG.Image.swift:303-321: CgBI?, IHDR
    s.ios = n && UNI(entries[0].type) == T_CgBI;
    const uint32_t at = s.ios;
    if (at < n && UNI(entries[at].type) == T_IHDR) {
        ParseScope first = s;
        first.depth = 8;                                       // (the header's own parser asks for no header)
        const spng_chunk_value h = parse_value(T_IHDR, p + uni64(entries[at].offset), UNI(entries[at].length), first, lane);
        if (lane == 0) vals[at] = h;
        r.ihdr_index = at;
        if (h.status == SPNG_DONE) { s.depth = h.v[2]; s.color = h.v[3]; r.interlaced = (uint8_t)h.v[4]; }
    }
    // the first PLTE
    uint32_t plte = SPNG_NO_OFFSET;
    for (uint64_t base = 0; base < n && plte == SPNG_NO_OFFSET; base += 64) {
        const uint64_t i = base + lane;
        const unsigned long long hit = __ballot(i < n && entries[i].type == T_PLTE);
        if (hit) plte = (uint32_t)base + (uint32_t)__ffsll((long long)hit) - 1;
    }
    if (plte != SPNG_NO_OFFSET) {
        const spng_chunk_value v = parse_value(T_PLTE, p + uni64(entries[plte].offset), UNI(entries[plte].length), s, lane);
        if (lane == 0) vals[plte] = v;
        r.plte_index = plte;
        if (v.scope == SPNG_SCOPE_PARSED && v.status == SPNG_DONE) r.palette_count = v.count;
    }
    r.depth = (uint8_t)s.depth; r.color = (uint8_t)s.color; r.ios = (uint8_t)s.ios;
    if (lane == 0) parsed[file] = r;
}

__global__ __launch_bounds__(64) void parse_value_kernel(const spng_file_desc *__restrict__ files, const spng_chunk_dir *__restrict__ dirs,
                                                         const spng_lexed *__restrict__ out, spng_chunk_value *const *__restrict__ values,
                                                         const spng_parsed *__restrict__ parsed)
{
    const int lane = threadIdx.x;
    const uint32_t file = blockIdx.y;
    const uint32_t chunks = UNI(out[file].chunks), cap = UNI(dirs[file].cap);
    const uint32_t n = chunks < cap ? chunks : cap;
    if (blockIdx.x >= n) return;
    const spng_chunk_entry *entries = (const spng_chunk_entry *)uni64((uint64_t)dirs[file].d_entries);
    spng_chunk_value *vals = (spng_chunk_value *)uni64((uint64_t)values[file]);
    const gbyte *p = (const gbyte *)uni64((uint64_t)files[file].d_png);
    const uint32_t ihdr = UNI(parsed[file].ihdr_index), plte = UNI(parsed[file].plte_index), palette_count = UNI(parsed[file].palette_count);
    ParseScope s;
    s.depth = UNI(parsed[file].depth); s.color = UNI(parsed[file].color); s.ios = UNI(parsed[file].ios);
    for (uint32_t i = blockIdx.x; i < n; i += gridDim.x) {
        if (i == ihdr || i == plte) continue;                  // (parse_scope_kernel's)
        s.palette = plte < i && palette_count != 0; s.palette_count = s.palette ? palette_count : 0;
        const spng_chunk_value r = parse_value(UNI(entries[i].type), p + uni64(entries[i].offset), UNI(entries[i].length), s, lane);
        if (lane == 0) vals[i] = r;
    }
}

__global__ __launch_bounds__(64) void parse_first_kernel(const spng_chunk_dir *__restrict__ dirs, const spng_lexed *__restrict__ out,
                                                         spng_chunk_value *const *__restrict__ values, spng_parsed *__restrict__ parsed)
{
    const int lane = threadIdx.x;
    const uint32_t file = blockIdx.x;
    const uint32_t chunks = UNI(out[file].chunks), cap = UNI(dirs[file].cap);
    const uint32_t n = chunks < cap ? chunks : cap;
    const spng_chunk_value *vals = (const spng_chunk_value *)uni64((uint64_t)values[file]);
    for (uint64_t base = 0; base < n; base += 64) {
        const uint64_t i = base + lane;
        const unsigned long long bad = __ballot(i < n && vals[i].status != SPNG_DONE);
        if (!bad) continue;
        const uint32_t first = (uint32_t)base + (uint32_t)__ffsll((long long)bad) - 1;
        if (lane == 0) {
            spng_parsed &r = parsed[file];
            r.status = vals[first].status; r.index = first; r.aux[0] = vals[first].aux[0]; r.aux[1] = vals[first].aux[1];
        }
        return;
    }
}

// ---- files that arrive in pieces (spng_lex_resume_batch) --------------------------------------------------------------------
// The reference's OnlineDecoding tutorial (Snippets/PNG/OnlineDecoding.swift) retries signature() and chunk() on truncatedSignature /
// truncatedChunkHeader / truncatedChunkBody until the bytes are there.  Here the loop's state lives on the device between the pushes:
// the chunk in progress, what of it has been summed and copied, the running CRC.  The same three kernels as above, started at the
// state's chunk: `lexr_walk_kernel` lists what is NEW with this push -- the chunks that became complete, and of the chunk the input
// ends in the bytes that arrived --, in pieces of LEX_PIECE_BYTES (geometry.hpp); `lexr_piece_kernel` sums and copies a piece per wave,
// the first piece of a chunk from the state's running CRC; `lexr_finish_kernel` folds the pieces of a chunk (crc(A || B) = crc(A) *
// x^(8 |B|) + crc(B), the algebra of crc_partial_kernel / crc32_fold), lets the first failure in file order decide and writes the
// state back.  After every push the answer is what the whole-file kernels above give for the same prefix.
static constexpr uint32_t LEX_MAGIC = 0x5258454cu, LEX_NONE = 0xffffffffu;
// between two pushes of a file; zero-filled in front of the first one
struct LexState {
    uint32_t magic, started;                    // LEX_MAGIC once a push has been seen; the signature has been checked
    uint64_t off;                               // the header of the chunk in progress
    uint64_t idat_len;                          // IDAT bytes whose chunks' checksums have been verified
    uint64_t summed, copied;                    // of the chunk in progress: bytes of type + data that are in `crc`, payload bytes copied
    uint32_t crc, chunks;                       // ... the CRC-32 over them (a finished value, as wave_crc32 takes it); chunks lexed in full
    uint32_t ihdr_at, plte_at, trns_at, cgbi_at;    // the chunk that set the fields of `last` (LEX_NONE: none has)
    uint32_t final, pad;                        // `last` is the result for good: SPNG_DONE or an error
    spng_lexed last;                            // the previous answer: IHDR fields, PLTE / tRNS places
};
// a listed piece: bytes [lo, hi) of a chunk's type + data to sum, bytes [clo, chi) of its payload to copy
struct LexPiece {
    uint64_t off, idat_off, lo, hi, clo, chi;
    uint32_t length, declared, computed, crc_in;    // computed: the first piece's from crc_in on, a raw (zero-initialised, un-finalised) one of the others
    uint32_t chunk, pieces, complete, next_multi;   // pieces: in a chunk's first piece, how many it has (0 in the others); next_multi: the next chunk of several
};
struct LexRWalk {
    uint32_t listed, stop_index; int32_t stop_status; uint32_t skip;        // skip: the walk's result stands as it is, the state too
    uint32_t started, pad;                      // the signature has been seen
    uint64_t stop_aux, stop_off, stop_idat;
    uint32_t bad, first_multi, ihdr_at, plte_at, trns_at, cgbi_at;
    uint32_t tail, tail_crc;                    // the chunk in progress: its first piece in the list (LEX_NONE: tail_crc is its CRC so far)
    uint64_t tail_summed, tail_copied;
    uint64_t n_summed, n_copied, n_headers;     // this push: bytes through the CRC, IDAT bytes copied, headers walked (spng_lex_resume_stats)
};

__global__ __launch_bounds__(64) void lexr_walk_kernel(const spng_file_desc *__restrict__ files, void *const *__restrict__ states,
                                                       spng_lexed *__restrict__ out, LexPiece *__restrict__ table,
                                                       const uint64_t *__restrict__ table_at, LexRWalk *__restrict__ walks)
{
    __shared__ uint32_t tab[CRC_TAB];
    const int lane = threadIdx.x;
    const spng_file_desc f = files[blockIdx.x];
    const gbyte *p = (const gbyte *)uni64((uint64_t)f.d_png);
    const uint64_t n = uni64(f.len);
    gbyte *idat = (gbyte *)uni64((uint64_t)f.d_idat);
    const uint64_t cap = uni64(f.idat_cap);
    LexPiece *list = table + uni64(table_at[blockIdx.x]);
    const uint32_t list_cap = (uint32_t)(uni64(table_at[blockIdx.x + 1]) - uni64(table_at[blockIdx.x]));
    const LexState *sp = (const LexState *)uni64((uint64_t)states[blockIdx.x]);
    spng_lexed r;
    memset(&r, 0, sizeof r);
    LexRWalk w;
    memset(&w, 0, sizeof w);
    w.stop_status = SPNG_DONE; w.bad = w.first_multi = w.tail = LEX_NONE;
    w.ihdr_at = w.plte_at = w.trns_at = w.cgbi_at = LEX_NONE;
    uint64_t off = 8, idat_len = 0, sum_from = 0, copy_from = 0;
    uint32_t index = 0, crc_in = 0;
    bool started = false, refuse = sp == nullptr;
    // the state: what the previous pushes left.  The host never looks into it, so what is wrong with it is this file's result
    if (!refuse && UNI(sp->magic) != 0) {
        const LexState s = *sp;
        const bool is_final = UNI(s.final) != 0;
        refuse = UNI(s.magic) != LEX_MAGIC || UNI(s.final) > 1 || UNI(s.started) > 1;
        started = UNI(s.started) != 0; off = uni64(s.off); idat_len = uni64(s.idat_len); sum_from = uni64(s.summed); copy_from = uni64(s.copied);
        crc_in = UNI(s.crc); index = UNI(s.chunks);
        if (!refuse && is_final && (s.last.status != SPNG_DONE || n >= off)) {
            // terminal and sticky: the answer again, nothing read (behind IEND: further bytes are ignored)
            w.skip = 1;
            if (lane == 0) { out[blockIdx.x] = s.last; walks[blockIdx.x] = w; }
            return;
        }
        // fields that contradict each other, or fewer bytes than the state has consumed
        refuse = refuse || is_final || (started ? off < 8 : (off | idat_len | sum_from | index) != 0);
        refuse = refuse || off > n || sum_from > n || idat_len > cap;      // (nothing below may wrap, nothing may be copied behind the buffer)
        refuse = refuse || (sum_from ? sum_from < 4 || copy_from + 4 > sum_from : (copy_from | crc_in) != 0);
        refuse = refuse || (s.ihdr_at != LEX_NONE && s.ihdr_at >= index) || (s.plte_at != LEX_NONE && s.plte_at >= index);
        refuse = refuse || (s.trns_at != LEX_NONE && s.trns_at >= index) || (s.cgbi_at != LEX_NONE && s.cgbi_at >= index);
        refuse = refuse || n < (started ? off + (sum_from ? 4 + sum_from : 0) : 0);
        if (!started) off = 8;
        r = s.last; r.status = 0; r.chunks = 0; r.aux[0] = r.aux[1] = 0; r.idat_len = r.consumed = 0;
        w.ihdr_at = s.ihdr_at; w.plte_at = s.plte_at; w.trns_at = s.trns_at; w.cgbi_at = s.cgbi_at;
    }
    // (the chunk in progress: its header is read again, and has to allow what the state says of it)
    if (!refuse && sum_from && (uint64_t)be32(p + off) + 4 < sum_from) refuse = true;
    if (UB(refuse)) {
        memset(&r, 0, sizeof r);
        r.status = SPNG_E_ARGUMENT; w.skip = 1;
        if (lane == 0) { out[blockIdx.x] = r; walks[blockIdx.x] = w; }
        return;
    }
    bool tabled = false;
    uint32_t listed = 0, last_multi = LEX_NONE;
    uint64_t n_summed = 0, n_copied = 0, n_headers = 0;
    // signature() (:44-56)
    if (!started) {
        if (n < 8) w.stop_status = SPNG_E_TRUNCATED_SIGNATURE;
        else {
            const uint64_t sig = (uint64_t)be32(p) << 32 | be32(p + 4);
            if (sig != 0x89504e470d0a1a0aull) { w.stop_status = SPNG_E_SIGNATURE; w.stop_aux = sig; }
            started = true;
        }
    }
    while (w.stop_status == SPNG_DONE) {
        // chunk() (:71-108), the checks of lex_walk_kernel in its order
        if (off + 8 > n) { w.stop_status = SPNG_E_TRUNCATED_CHUNK_HEADER; break; }
        n_headers += 1;
        const uint32_t length = be32(p + off), name = be32(p + off + 4);
        if (!valid_type(name)) { w.stop_status = SPNG_E_CHUNK_TYPE; w.stop_aux = name; break; }
        const uint64_t bytes = (uint64_t)length + 4;
        const bool complete = off + 8 + bytes <= n;
        const uint64_t avail = n - off - 4 < bytes ? n - off - 4 : bytes;     // bytes of type + data that are there (at least the type)
        const uint64_t fresh = avail - sum_from;
        const gbyte *data = p + off + 8;
        const bool copies = name == 0x49444154 && idat_len + length <= cap;
        const uint64_t chi = copies ? avail - 4 : copy_from;
        w.tail_crc = crc_in;
        if (complete && name == 0x49444154 && !copies) {
            // (the reference's order: the checksum first)
            if (!tabled) { crc_table(tab, lane); tabled = true; }
            const uint32_t declared = be32(data + length), computed = wave_crc32(tab, p + off + 4 + sum_from, fresh, crc_in, lane);
            n_summed += fresh;
            if (declared != computed) { w.stop_status = SPNG_E_CHUNK_CHECKSUM; w.stop_aux = (uint64_t)declared << 32 | computed; }
            else w.stop_status = SPNG_E_OUTPUT_CAPACITY;
            break;
        }
        const uint64_t q = lex_resume_pieces(fresh, complete);
        if (q && listed + q <= list_cap) {
            const uint32_t declared = complete ? be32(data + length) : 0;
            for (uint64_t j = lane; j < q; j += 64) {
                LexPiece c;
                c.off = off; c.idat_off = idat_len;
                c.lo = sum_from + j * LEX_PIECE_BYTES; c.hi = c.lo + LEX_PIECE_BYTES < avail ? c.lo + LEX_PIECE_BYTES : avail;
                c.clo = j ? c.lo - 4 : copy_from; c.chi = copies ? c.hi - 4 : c.clo;
                c.length = length; c.declared = declared; c.computed = 0; c.crc_in = crc_in;
                c.chunk = index; c.pieces = j ? 0 : (uint32_t)q; c.complete = complete; c.next_multi = LEX_NONE;
                list[listed + j] = c;
            }
            if (q > 1) {
                if (last_multi == LEX_NONE) w.first_multi = listed;
                else if (lane == 0) list[last_multi].next_multi = listed;
                last_multi = listed;
            }
            if (!complete) w.tail = listed;
            listed += (uint32_t)q;
            n_summed += fresh; n_copied += chi - copy_from;
        } else if (q) {
            // the list is full: this wave sums and copies the chunk itself
            if (!tabled) { crc_table(tab, lane); tabled = true; }
            const uint32_t computed = wave_crc32(tab, p + off + 4 + sum_from, fresh, crc_in, lane);
            n_summed += fresh;
            if (complete) {
                const uint32_t declared = be32(data + length);
                if (declared != computed) { w.stop_status = SPNG_E_CHUNK_CHECKSUM; w.stop_aux = (uint64_t)declared << 32 | computed; break; }
            }
            copy_bytes(idat + idat_len + copy_from, data + copy_from, chi - copy_from, lane);
            n_copied += chi - copy_from;
            w.tail_crc = computed;
        }
        if (!complete) {
            w.stop_status = SPNG_E_TRUNCATED_CHUNK_BODY; w.stop_aux = bytes;
            w.tail_summed = avail; w.tail_copied = chi;
            break;
        }
        if (name == 0x43674249) w.cgbi_at = w.cgbi_at == LEX_NONE ? index : w.cgbi_at;
        else if (name == 0x49484452 && length >= 13) {
            r.width = be32(data); r.height = be32(data + 4);
            r.depth = data[8]; r.color = data[9]; r.compression = data[10]; r.filter = data[11]; r.interlace = data[12];
            w.ihdr_at = index;
        } else if (name == 0x504c5445) { r.plte_off = off + 8; r.plte_len = length; w.plte_at = index; }
        else if (name == 0x74524e53) { r.trns_off = off + 8; r.trns_len = length; w.trns_at = index; }
        else if (name == 0x49444154) idat_len += length;
        index += 1;
        off += 8 + bytes;
        sum_from = copy_from = 0; crc_in = 0;
        if (name == 0x49454e44) break;                         // IEND
    }
    w.listed = listed; w.started = started;
    w.stop_index = index; w.stop_off = off; w.stop_idat = idat_len;
    w.n_summed = n_summed; w.n_copied = n_copied; w.n_headers = n_headers;
    if (lane == 0) { out[blockIdx.x] = r; walks[blockIdx.x] = w; }
}

__global__ __launch_bounds__(64) void lexr_piece_kernel(const spng_file_desc *__restrict__ files, LexPiece *__restrict__ table,
                                                        const uint64_t *__restrict__ table_at, LexRWalk *__restrict__ walks)
{
    __shared__ uint32_t tab[CRC_TAB];
    const int lane = threadIdx.x;
    const uint32_t file = blockIdx.y;
    const uint32_t listed = UNI(walks[file].listed);
    if (blockIdx.x >= listed || UNI(walks[file].skip)) return;
    const spng_file_desc f = files[file];
    const gbyte *p = (const gbyte *)uni64((uint64_t)f.d_png);
    gbyte *idat = (gbyte *)uni64((uint64_t)f.d_idat);
    LexPiece *list = table + uni64(table_at[file]);
    crc_table(tab, lane);
    for (uint32_t k = blockIdx.x; k < listed; k += gridDim.x) {
        const uint64_t off = uni64(list[k].off), lo = uni64(list[k].lo), hi = uni64(list[k].hi);
        const uint64_t clo = uni64(list[k].clo), chi = uni64(list[k].chi);
        const uint32_t pieces = UNI(list[k].pieces);
        uint32_t computed;
        if (pieces) computed = wave_crc32(tab, p + off + 4 + lo, hi - lo, UNI(list[k].crc_in), lane);
        else {
            computed = crc32_conditioning(wave_crc32(tab, p + off + 4 + lo, hi - lo, 0, lane), hi - lo);       // (a raw one, as crc_partial_kernel's)
        }
        // (the payload is copied ahead of the chunk's checksum: idat_len moves on only once that has been verified)
        if (chi > clo) copy_bytes(idat + uni64(list[k].idat_off) + clo, p + off + 8 + clo, chi - clo, lane);
        const uint32_t declared = UNI(list[k].declared);
        const bool decides = pieces == 1 && UNI(list[k].complete) != 0;     // (chunks of several pieces: the finish folds and compares)
        if (lane == 0) {
            list[k].computed = computed;
            if (decides && computed != declared) atomicMin(&walks[file].bad, k);
        }
    }
}

__global__ void lexr_finish_kernel(spng_lexed *__restrict__ out, LexPiece *__restrict__ table, const uint64_t *__restrict__ table_at,
                                   const LexRWalk *__restrict__ walks, const spng_file_desc *__restrict__ files, void *const *__restrict__ states,
                                   unsigned long long *__restrict__ stats, uint32_t count)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    // the call's counters: a wave adds up its files', an atomic per wave (one per file on one address: a call over 8192 small files
    // 0.43 ms instead of 0.20).  Every lane of the wave arrives here
    unsigned long long sums[3] = {0, 0, 0};
    if (i < count) { sums[0] = walks[i].n_summed; sums[1] = walks[i].n_copied; sums[2] = walks[i].n_headers; }
    for (int k = 0; k < 3; ++k) {
        if (__ballot(sums[k] != 0) == 0) continue;
        unsigned long long total = sums[k];
#pragma unroll
        for (int m = 32; m; m >>= 1) {
            const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)total, m), hi = (uint32_t)__shfl_xor((int)(uint32_t)(total >> 32), m);
            total += (unsigned long long)hi << 32 | lo;
        }
        if ((threadIdx.x & 63) == 0) atomicAdd(stats + k, total);
    }
    if (i >= count) return;
    const LexRWalk w = walks[i];
    if (w.skip) return;
    LexPiece *list = table + table_at[i];
    // the chunks of several pieces: folded, and compared if they are complete
    uint32_t bad = w.bad;
    for (uint32_t e = w.first_multi; e != LEX_NONE; e = list[e].next_multi) {
        uint32_t c = list[e].computed ^ 0xffffffffu;
        for (uint32_t j = 1; j < list[e].pieces; ++j) c = multmodp(xpow8(list[e + j].hi - list[e + j].lo), c) ^ list[e + j].computed;
        list[e].computed = c ^ 0xffffffffu;
        if (list[e].complete && list[e].computed != list[e].declared && e < bad) bad = e;
    }
    spng_lexed r = out[i];
    uint32_t upto = w.stop_index;                              // chunks lexed in full
    r.status = w.stop_status;
    if (w.stop_status == SPNG_E_CHUNK_CHECKSUM) { r.aux[0] = w.stop_aux >> 32; r.aux[1] = (uint32_t)w.stop_aux; }
    else r.aux[0] = w.stop_aux;
    r.consumed = w.stop_off; r.idat_len = w.stop_idat;
    if (bad != LEX_NONE) {
        // a checksum failed in front of whatever stopped the walk
        const LexPiece c = list[bad];
        upto = c.chunk;
        r.status = SPNG_E_CHUNK_CHECKSUM; r.aux[0] = c.declared; r.aux[1] = c.computed;
        r.consumed = c.off; r.idat_len = c.idat_off;
    }
    r.chunks = upto;
    // what lies behind the first failure was never seen by the reference's loop
    if (w.ihdr_at >= upto) { r.width = r.height = 0; r.depth = r.color = r.compression = r.filter = r.interlace = 0; }
    if (w.plte_at >= upto) { r.plte_off = 0; r.plte_len = 0; }
    if (w.trns_at >= upto) { r.trns_off = 0; r.trns_len = 0; }
    r.ios = w.cgbi_at != LEX_NONE && w.cgbi_at < upto ? 1 : 0;
    if (r.consumed > files[i].len) r.consumed = files[i].len;
    out[i] = r;
    // the state: the three truncations wait for more; everything else is final, written once
    LexState s;
    memset(&s, 0, sizeof s);
    const bool waits = r.status == SPNG_E_TRUNCATED_SIGNATURE || r.status == SPNG_E_TRUNCATED_CHUNK_HEADER || r.status == SPNG_E_TRUNCATED_CHUNK_BODY;
    s.magic = LEX_MAGIC; s.started = w.started; s.final = waits ? 0 : 1;
    s.off = s.started ? w.stop_off : 0; s.idat_len = w.stop_idat; s.chunks = w.stop_index;
    if (r.status == SPNG_E_TRUNCATED_CHUNK_BODY) {
        s.summed = w.tail_summed; s.copied = w.tail_copied;
        s.crc = w.tail != LEX_NONE ? list[w.tail].computed : w.tail_crc;
    }
    s.ihdr_at = w.ihdr_at; s.plte_at = w.plte_at; s.trns_at = w.trns_at; s.cgbi_at = w.cgbi_at;
    s.last = r;
    *(LexState *)states[i] = s;
}

// PNG.BytestreamDestination.format(type: .IDAT, data:) for every piece of a stream (:66-88)
__global__ __launch_bounds__(64) void write_idat_kernel(const spng_chunking_desc *__restrict__ descs, spng_result *__restrict__ results)
{
    __shared__ uint32_t tab[CRC_TAB];
    const int lane = threadIdx.x;
    const spng_chunking_desc d = descs[blockIdx.y];
    const uint64_t n = uni64(d.len), piece = uni64(d.chunk_bytes);
    const uint64_t pieces = n ? (n + piece - 1) / piece : 0;
    const uint64_t need = n + 12 * pieces;
    if (blockIdx.x == 0 && lane == 0) {
        spng_result &res = results[blockIdx.y];
        res.status = need > d.out_cap ? SPNG_E_OUTPUT_CAPACITY : SPNG_DONE; res.reserved = 0;
        res.written = need; res.consumed = n; res.aux[0] = pieces; res.aux[1] = 0;
    }
    if (need > d.out_cap) return;
    crc_table(tab, lane);
    const gbyte *src = (const gbyte *)uni64((uint64_t)d.d_stream);
    gbyte *out = (gbyte *)uni64((uint64_t)d.d_out);
    for (uint64_t k = blockIdx.x; k < pieces; k += gridDim.x) {
        const uint64_t lo = k * piece, len = n - lo < piece ? n - lo : piece;
        gbyte *o = out + lo + 12 * k;
        if (lane < 4) o[lane] = (uint8_t)(len >> (8 * (3 - lane)));
        if (lane < 4) o[4 + lane] = (uint8_t)(0x49444154u >> (8 * (3 - lane)));
        for (uint64_t i = lane; i < len; i += 64) o[8 + i] = src[lo + i];
        const uint32_t crc = chunk_crc32(tab, 0x49444154u, src + lo, len, lane);
        if (lane < 4) o[8 + len + lane] = (uint8_t)(crc >> (8 * (3 - lane)));
    }
}

// ---- whole files (spng_write_file_batch) ------------------------------------------------------------------------------------
// PNG.Image.compress(stream:level:hint:) behind its encoder (PNG.Image.swift:576-668): signature ‖ head ‖ IDAT chunks ‖ IEND.  The head
// -- everything between the signature and the first IDAT -- arrives finished from the host (file_head.hpp).  The stream's length is a
// host value or the `written` of a spng_result the deflater left in device memory, so no launch depends on it: the grid is sized by
// the stream's capacity, a wave strides over the units of its file (geometry.hpp: a unit is a piece of at most FILE_PIECE_BYTES of a
// chunk) and the waves without a unit leave.  `wfile_body_kernel`: a unit is copied -- 16-byte stores aligned on the DESTINATION, whose
// offset against the source changes from chunk to chunk (8 + head + k (c + 12) + 8 against k c), unaligned 16-byte loads, the bytes
// in front of the first and behind the last aligned unit by the lanes they belong to -- and summed from the source by wave_crc32; a
// chunk of one piece is finished there, the raw sums of a longer one go to `wfile_finish_kernel`, a thread per chunk, which folds
// them (crc(A || B) = crc(A) * x^(8 |B|) + crc(B): every piece but the last is FILE_PIECE_BYTES long, one constant of CRC_POW).
__device__ __forceinline__ void copy_dst_aligned(gbyte *dst, const gbyte *src, uint64_t n, int lane)
{
    typedef uint32_t c4 __attribute__((vector_size(16)));
    struct __attribute__((packed)) P16 { c4 v; };
    typedef P16 __attribute__((address_space(1))) gP16;
    typedef c4 __attribute__((address_space(1))) gA16;
    const uint64_t lead = (16 - ((uint64_t)dst & 15)) & 15, head = lead < n ? lead : n;
    if ((uint64_t)lane < head) dst[lane] = src[lane];
    const uint64_t units = (n - head) / 16;
    // (eight loads in flight per lane: a piece of 1 MiB is one wave's, and a load a step left it waiting on memory 1024 times)
    uint64_t u = lane;
    for (; u + 7 * 64 < units; u += 8 * 64) {
        c4 v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = ((const gP16 *)(src + head + (u + 64 * k) * 16))->v;
#pragma unroll
        for (int k = 0; k < 8; ++k) *(gA16 *)(dst + head + (u + 64 * k) * 16) = v[k];
    }
    for (; u < units; u += 64) *(gA16 *)(dst + head + u * 16) = ((const gP16 *)(src + head + u * 16))->v;
    const uint64_t done = head + units * 16;
    if ((uint64_t)lane < n - done) dst[done + lane] = src[done + lane];
}

// what a file's result says before anything is written: the length, the chunks, the bytes needed
struct FilePlan { int32_t status; uint64_t n, chunks, need, aux0, aux1; };
__device__ __forceinline__ FilePlan wfile_plan(const FileJob &j)
{
    FilePlan p;
    p.status = SPNG_DONE; p.n = uni64(j.len); p.chunks = p.need = p.aux0 = p.aux1 = 0;
    const spng_result *sr = (const spng_result *)uni64((uint64_t)j.src_result);
    if (sr) {
        p.status = (int32_t)UNI(sr->status); p.n = uni64(sr->written);
        if (p.status != SPNG_DONE) { p.aux0 = uni64(sr->aux[0]); p.aux1 = uni64(sr->aux[1]); return p; }
    }
    // (no zlib stream is empty; a length behind the capacity the launch and the scratch were sized by is nobody's stream)
    if (p.n == 0 || p.n > uni64(j.stream_cap)) { p.status = SPNG_E_ARGUMENT; return p; }
    p.chunks = file_chunks(p.n, uni64(j.chunk_bytes));
    p.need = 8 + uni64(j.head_len) + p.n + 12 * p.chunks + 12;
    if (p.need > uni64(j.out_cap)) p.status = SPNG_E_OUTPUT_CAPACITY;
    return p;
}

__global__ __launch_bounds__(64) void wfile_body_kernel(const FileJob *__restrict__ jobs, spng_result *__restrict__ results)
{
    __shared__ uint32_t tab[CRC_TAB];
    const int lane = threadIdx.x;
    const FileJob j = jobs[blockIdx.y];
    const FilePlan p = wfile_plan(j);
    if (blockIdx.x == 0 && lane == 0) {
        spng_result &res = results[blockIdx.y];
        res.status = p.status; res.reserved = 0;
        res.written = p.status == SPNG_DONE || p.status == SPNG_E_OUTPUT_CAPACITY ? p.need : 0;
        res.consumed = p.status == SPNG_DONE ? p.n : 0;
        res.aux[0] = p.status == SPNG_DONE ? p.chunks : p.aux0; res.aux[1] = p.aux1;
    }
    if (p.status != SPNG_DONE) return;
    const uint64_t c = uni64(j.chunk_bytes), head_len = uni64(j.head_len);
    const uint64_t per = file_pieces(c), full = (p.chunks - 1) * per, units = full + file_pieces(p.n - (p.chunks - 1) * c);
    if (blockIdx.x >= units) return;
    const gbyte *stream = (const gbyte *)uni64((uint64_t)j.stream);
    gbyte *out = (gbyte *)uni64((uint64_t)j.out);
    uint32_t *partial = (uint32_t *)uni64((uint64_t)j.partial);
    if (blockIdx.x == 0) {
        // signature() and the head in front of the chunks, format(type: .IEND) behind them (BytestreamDestination.swift:44-88)
        if (lane < 8) out[lane] = (uint8_t)(0x89504e470d0a1a0aull >> (8 * (7 - lane)));
        copy_dst_aligned(out + 8, (const gbyte *)uni64((uint64_t)j.head), head_len, lane);
        if (lane < 12) out[p.need - 12 + lane] = (uint8_t)(lane < 4 ? 0 : (0x49454e44ae426082ull >> (8 * (11 - lane))));
    }
    crc_table(tab, lane);
    for (uint64_t u = blockIdx.x; u < units; u += gridDim.x) {
        const uint64_t k = u < full ? u / per : p.chunks - 1, piece = u < full ? u % per : u - full;
        const uint64_t clen = k == p.chunks - 1 ? p.n - k * c : c;
        const uint64_t lo = piece * FILE_PIECE_BYTES, len = clen - lo < FILE_PIECE_BYTES ? clen - lo : FILE_PIECE_BYTES;
        const gbyte *src = stream + k * c + lo;
        gbyte *o = out + 8 + head_len + k * (c + 12);
        copy_dst_aligned(o + 8 + lo, src, len, lane);
        if (piece == 0 && lane < 8) o[lane] = (uint8_t)(((uint64_t)clen << 32 | 0x49444154u) >> (8 * (7 - lane)));
        if (clen <= FILE_PIECE_BYTES) {
            const uint32_t crc = chunk_crc32(tab, 0x49444154u, src, len, lane);
            if (lane < 4) o[8 + clen + lane] = (uint8_t)(crc >> (8 * (3 - lane)));
        } else {
            // raw sums: the first piece's over the type and its bytes
            const uint32_t raw = piece == 0 ? crc32_conditioning(chunk_crc32(tab, 0x49444154u, src, len, lane), len + 4)
                                            : crc32_conditioning(wave_crc32(tab, src, len, 0, lane), len);
            if (lane == 0) partial[u] = raw;
        }
    }
}

// the chunks of several pieces: folded and written, a thread per chunk
__global__ void wfile_finish_kernel(const FileJob *__restrict__ jobs, const spng_result *__restrict__ results)
{
    const FileJob j = jobs[blockIdx.y];
    const spng_result r = results[blockIdx.y];
    if (r.status != SPNG_DONE || j.chunk_bytes <= FILE_PIECE_BYTES) return;
    const uint64_t c = j.chunk_bytes, n = r.consumed, chunks = r.aux[0], per = file_pieces(c);
    for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < chunks; k += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t clen = k == chunks - 1 ? n - k * c : c;
        if (clen <= FILE_PIECE_BYTES) continue;                // (finished by the wave that copied it)
        const uint64_t pieces = file_pieces(clen);
        const uint32_t *part = j.partial + k * per;
        uint32_t crc = part[0];
        for (uint64_t q = 1; q < pieces; ++q)
            crc = multmodp(q + 1 < pieces ? CRC_POW.v[20] : xpow8(clen - q * FILE_PIECE_BYTES), crc) ^ part[q];
        crc = crc32_conditioning(crc, clen + 4);
        uint8_t *o = j.out + 8 + j.head_len + k * (c + 12) + 8 + clen;
        for (int b = 0; b < 4; ++b) o[b] = (uint8_t)(crc >> (8 * (3 - b)));
    }
}
static_assert(FILE_PIECE_BYTES == 1ull << 20, "wfile_finish_kernel shifts by CRC_POW.v[20]");

// raw (zero-initialised, un-finalised) CRC of 1 MiB pieces: the host folds them (spng_crc32)
__global__ __launch_bounds__(64) void crc_partial_kernel(const uint8_t *__restrict__ data, uint64_t n, uint64_t piece, uint32_t *__restrict__ partial)
{
    __shared__ uint32_t tab[CRC_TAB];
    const int lane = threadIdx.x;
    crc_table(tab, lane);
    const uint64_t lo = (uint64_t)blockIdx.x * piece, len = n - lo < piece ? n - lo : piece;
    const uint32_t std_crc = wave_crc32(tab, (const gbyte *)data + lo, len, 0, lane);
    if (lane == 0) partial[blockIdx.x] = crc32_conditioning(std_crc, len);
}

uint32_t crc32_fold(const uint32_t *partial, uint64_t pieces, uint64_t n, uint64_t piece)
{
    uint32_t c = 0;
    for (uint64_t k = 0; k < pieces; ++k) {
        const uint64_t len = n - k * piece < piece ? n - k * piece : piece;
        c = multmodp(xpow8(len), c) ^ partial[k];
    }
    return crc32_conditioning(c, n);
}

size_t lex_chunk_bytes() { return sizeof(LexChunk); }
size_t lex_walk_bytes() { return sizeof(LexWalk); }
hipError_t launch_lex(const spng_file_desc *d_files, uint32_t count, spng_lexed *d_out, void *d_table, const uint64_t *d_table_at,
                      void *d_walks, uint32_t max_listed, hipStream_t stream)
{
    if (!count) return hipSuccess;
    lex_walk_kernel<<<count, 64, 0, stream>>>(d_files, d_out, (LexChunk *)d_table, d_table_at, (LexWalk *)d_walks);
    const uint32_t bx = lex_piece_blocks_x(count, max_listed);
    const hipError_t e = launch_rows(count, [&](uint32_t y0, uint32_t ny) {
        lex_chunk_kernel<<<dim3(bx, ny), 64, 0, stream>>>(d_files + y0, (LexChunk *)d_table, d_table_at + y0, (LexWalk *)d_walks + y0);
    });
    if (e != hipSuccess) return e;
    lex_finish_kernel<<<(count + 63) / 64, 64, 0, stream>>>(d_out, (const LexChunk *)d_table, d_table_at, (const LexWalk *)d_walks, d_files, count);
    return hipGetLastError();
}
// behind launch_lex on the same stream.  most_entries: the most entries a file of the call can get
hipError_t launch_lex_dir(const spng_file_desc *d_files, const spng_chunk_dir *d_dirs, uint32_t count, const spng_lexed *d_out, const void *d_table,
                          const uint64_t *d_table_at, const void *d_walks, uint32_t most_entries, hipStream_t stream)
{
    if (!count || !most_entries) return hipSuccess;
    dir_list_kernel<<<count, 64, 0, stream>>>(d_files, d_dirs, d_out, (const LexChunk *)d_table, d_table_at, (const LexWalk *)d_walks);
    const uint32_t bx = lex_piece_blocks_x(count, most_entries);
    return launch_rows(count, [&](uint32_t y0, uint32_t ny) {
        dir_head_kernel<<<dim3(bx, ny), 64, 0, stream>>>(d_files + y0, d_dirs + y0, d_out + y0);
    });
}
hipError_t launch_parse_dir(const spng_file_desc *d_files, const spng_chunk_dir *d_dirs, uint32_t count, const spng_lexed *d_infos,
                            spng_chunk_value *const *d_values, uint32_t most_entries, spng_parsed *d_parsed, hipStream_t stream)
{
    if (!count) return hipSuccess;
    parse_scope_kernel<<<count, 64, 0, stream>>>(d_files, d_dirs, d_infos, d_values, d_parsed);
    if (most_entries) {
        const uint32_t bx = lex_piece_blocks_x(count, most_entries);
        const hipError_t e = launch_rows(count, [&](uint32_t y0, uint32_t ny) {
            parse_value_kernel<<<dim3(bx, ny), 64, 0, stream>>>(d_files + y0, d_dirs + y0, d_infos + y0, d_values + y0, d_parsed + y0);
        });
        if (e != hipSuccess) return e;
    }
    parse_first_kernel<<<count, 64, 0, stream>>>(d_dirs, d_infos, d_values, d_parsed);
    return hipGetLastError();
}
size_t lex_state_bytes() { return sizeof(LexState); }
size_t lex_piece_bytes() { return sizeof(LexPiece); }
size_t lex_rwalk_bytes() { return sizeof(LexRWalk); }
hipError_t launch_lex_resume(const spng_file_desc *d_files, void *const *d_states, uint32_t count, spng_lexed *d_out, void *d_table,
                             const uint64_t *d_table_at, void *d_walks, uint32_t max_listed, uint64_t *d_stats, hipStream_t stream)
{
    if (!count) return hipSuccess;
    lexr_walk_kernel<<<count, 64, 0, stream>>>(d_files, d_states, d_out, (LexPiece *)d_table, d_table_at, (LexRWalk *)d_walks);
    const uint32_t bx = lex_piece_blocks_x(count, max_listed);
    const hipError_t e = launch_rows(count, [&](uint32_t y0, uint32_t ny) {
        lexr_piece_kernel<<<dim3(bx, ny), 64, 0, stream>>>(d_files + y0, (LexPiece *)d_table, d_table_at + y0, (LexRWalk *)d_walks + y0);
    });
    if (e != hipSuccess) return e;
    lexr_finish_kernel<<<(count + 63) / 64, 64, 0, stream>>>(d_out, (LexPiece *)d_table, d_table_at, (const LexRWalk *)d_walks, d_files, d_states,
                                                                 (unsigned long long *)d_stats, count);
    return hipGetLastError();
}
hipError_t launch_write_idat(const spng_chunking_desc *d_descs, uint32_t count, uint32_t blocks_x, spng_result *d_results, hipStream_t stream)
{
    if (!count) return hipSuccess;
    return launch_rows(count, [&](uint32_t y0, uint32_t ny) {
        write_idat_kernel<<<dim3(blocks_x ? blocks_x : 1, ny), 64, 0, stream>>>(d_descs + y0, d_results + y0);
    });
}
hipError_t launch_write_file(const FileJob *d_jobs, uint32_t count, uint32_t blocks_x, uint64_t finish_chunks, spng_result *d_results,
                             hipStream_t stream)
{
    if (!count) return hipSuccess;
    const hipError_t e = launch_rows(count, [&](uint32_t y0, uint32_t ny) {
        wfile_body_kernel<<<dim3(blocks_x ? blocks_x : 1, ny), 64, 0, stream>>>(d_jobs + y0, d_results + y0);
    });
    if (e != hipSuccess || !finish_chunks) return e;
    const uint32_t fx = (uint32_t)std::min<uint64_t>((finish_chunks + 63) / 64, 1024);
    return launch_rows(count, [&](uint32_t y0, uint32_t ny) {
        wfile_finish_kernel<<<dim3(fx, ny), 64, 0, stream>>>(d_jobs + y0, d_results + y0);
    });
}
hipError_t launch_crc_partial(const uint8_t *d, uint64_t n, uint64_t piece, uint32_t *d_partial, uint32_t pieces, hipStream_t stream)
{
    if (!pieces) return hipSuccess;
    crc_partial_kernel<<<pieces, 64, 0, stream>>>(d, n, piece, d_partial);
    return hipGetLastError();
}

}  // namespace spng
