// emu_metadata.cpp -- TEST INFRASTRUCTURE: runs the kernels of the chunk directory (csrc/chunks.hip: lex_walk -> lex_chunk -> lex_finish ->
// dir_list -> dir_head) and of the text entry (csrc/text.hip: text_count -> text_scan -> text_write) on the CPU
// (tools/emu/hip/hip_runtime.h), from prepared copies of the sources as written (EMU_CHUNKS_SRC, EMU_TEXT_SRC: launches blanked).  It prints
// what the kernels answer; the yardstick is the test's (tests/metadata_ref.py).  Built and used by tests/test_emu_metadata.py, never part
// of the product.  Every input is handed over as a copy of exactly its bytes, every output as a buffer of exactly its capacity
// between guard bytes that are looked at afterwards, so that a sanitizer build sees a read or write past an end and a plain build a
// write.
//
//   emu_metadata <blob file> <script file> <out file>
// script, a command per line (offsets and lengths are into the blob file):
//   blocks <n>                          workgroups along x of the per-chunk and per-tile kernels (default 3)
//   dir <off> <len> <cap> <list>        the file blob[off, off + len) lexed with a directory of `cap` entries; list: capacity of the lexer's
//                                       list (-1: lex_listed).  Prints
//       L status chunks aux0 aux1 width height depth color compression filter interlace ios idat_len plte_off plte_len trns_off trns_len consumed pad0 pad1
//       E type length offset status aux k l m body_off compressed pad      per entry in front of min(chunks, cap) (pad: the sum of its padding bytes)
//       G untouched                     1: the entries behind them and the guard bytes are as they were
//   head <type> <off> <len>             dir_head_kernel alone over the payload blob[off, off + len) as a file of exactly those bytes.  Prints
//       H status aux k l m body_off compressed
//   text <op> <off> <len> <src_at> <dst_at> <out_cap>      the text blob[off, off + len), source and destination so many bytes behind a
//                                       16-byte boundary.  Prints
//       T status written consumed aux0 aux1 guards
//     and, transcoding with SPNG_DONE, appends the bytes written to the out file
#include EMU_CHUNKS_SRC
#include EMU_TEXT_SRC

#include <fstream>
#include <iostream>
#include <sstream>
#include <vector>

using namespace spng;

static std::vector<uint8_t> slurp(const char *path)
{
    std::ifstream f(path, std::ios::binary);
    return std::vector<uint8_t>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

static constexpr size_t GUARD = 32;
// `n` bytes `at` bytes behind a 16-byte boundary, GUARD bytes of 0xA5 on either side
struct Guarded {
    uint8_t *raw, *p; size_t n;
    Guarded(size_t n_, size_t at) : n(n_)
    {
        if (posix_memalign((void **)&raw, 64, 64 + at + n + GUARD)) abort();
        memset(raw, 0xA5, 64 + at + n + GUARD);
        p = raw + 64 + at;
    }
    bool intact() const
    {
        for (size_t i = 1; i <= GUARD; ++i) if (p[-(ptrdiff_t)i] != 0xA5) return false;
        for (size_t i = 0; i < GUARD; ++i) if (p[n + i] != 0xA5) return false;
        return true;
    }
    ~Guarded() { free(raw); }
};
// exactly n bytes, `at` bytes behind a 16-byte boundary: a sanitizer build sees a read behind them (and one in front of `at` = 0)
struct Exact {
    uint8_t *raw, *p;
    Exact(const uint8_t *src, size_t n, size_t at)
    {
        if (posix_memalign((void **)&raw, 16, at + n ? at + n : 1)) abort();
        memset(raw, 0xE2, at);                                  // (a lead byte: a look in front of the text would change the answer)
        p = raw + at;
        if (n) memcpy(p, src, n);
    }
    ~Exact() { free(raw); }
};

int main(int argc, char **argv)
{
    if (argc < 4) return 2;
    const std::vector<uint8_t> blob = slurp(argv[1]);
    std::ifstream script(argv[2]);
    std::ofstream out_file(argv[3], std::ios::binary);
    uint32_t blocks = 3;
    std::string line;
    while (std::getline(script, line)) {
        std::istringstream in(line);
        std::string cmd;
        in >> cmd;
        if (cmd == "blocks") in >> blocks;
        else if (cmd == "dir") {
            uint64_t off, n, cap; int64_t list_cap;
            in >> off >> n >> cap >> list_cap;
            if (off + n > blob.size()) return 3;
            Exact file(blob.data() + off, n, 0);
            std::vector<uint8_t> idat(n ? n : 1, 0xEE);
            spng_file_desc f{file.p, n, idat.data(), n};
            const uint64_t listed = list_cap >= 0 ? (uint64_t)list_cap : lex_listed(n);
            uint64_t table_at[2] = {0, listed};
            std::vector<LexChunk> table(listed + 1);
            LexWalk walk;
            spng_lexed info;
            memset(&info, 0, sizeof info);
            Guarded ent((cap + 2) * sizeof(spng_chunk_entry), 0);
            memset(ent.p, 0xEE, ent.n);
            spng_chunk_dir dir{cap ? (spng_chunk_entry *)ent.p : nullptr, (uint32_t)cap, 0};
            emu::launch(1, 64, [&] { lex_walk_kernel(&f, &info, table.data(), table_at, &walk); });
            emu::launch(blocks, 64, [&] { lex_chunk_kernel(&f, table.data(), table_at, &walk); }, 1);
            emu::launch(1, 64, [&] { lex_finish_kernel(&info, table.data(), table_at, &walk, &f, 1); });
            emu::launch(1, 64, [&] { dir_list_kernel(&f, &dir, &info, table.data(), table_at, &walk); });
            emu::launch(blocks, 64, [&] { dir_head_kernel(&f, &dir, &info); }, 1);
            printf("L %d %u %llx %llx %u %u %u %u %u %u %u %u %llu %llu %u %llu %u %llu %u %u\n", info.status, info.chunks, (unsigned long long)info.aux[0],
                   (unsigned long long)info.aux[1], info.width, info.height, info.depth, info.color, info.compression, info.filter, info.interlace, info.ios,
                   (unsigned long long)info.idat_len, (unsigned long long)info.plte_off, info.plte_len, (unsigned long long)info.trns_off, info.trns_len,
                   (unsigned long long)info.consumed, info.pad[0], info.pad[1]);
            const uint64_t filled = info.chunks < cap ? info.chunks : cap;
            const spng_chunk_entry *e = (const spng_chunk_entry *)ent.p;
            for (uint64_t i = 0; i < filled; ++i) {
                unsigned pad = 0;
                for (uint8_t b : e[i].pad) pad += b;
                printf("E %u %u %llu %d %u %u %u %u %u %u %u\n", e[i].type, e[i].length, (unsigned long long)e[i].offset, e[i].status, e[i].aux, e[i].k,
                       e[i].l, e[i].m, e[i].body_off, e[i].compressed, pad);
            }
            bool untouched = ent.intact();
            for (size_t i = filled * sizeof(spng_chunk_entry); i < ent.n; ++i) untouched = untouched && ent.p[i] == 0xEE;
            printf("G %d\n", untouched ? 1 : 0);
        } else if (cmd == "head") {
            std::string type; uint64_t off, n;
            in >> type >> off >> n;
            if (off + n > blob.size() || type.size() != 4) return 3;
            Exact payload(blob.data() + off, n, 0);
            spng_file_desc f{payload.p, n, nullptr, 0};
            spng_lexed info;
            memset(&info, 0, sizeof info);
            info.chunks = 1;
            spng_chunk_entry e;
            memset(&e, 0, sizeof e);
            e.type = (uint32_t)(uint8_t)type[0] << 24 | (uint32_t)(uint8_t)type[1] << 16 | (uint32_t)(uint8_t)type[2] << 8 | (uint8_t)type[3];
            e.length = (uint32_t)n; e.offset = 0; e.k = e.l = e.m = SPNG_NO_OFFSET;
            spng_chunk_dir dir{&e, 1, 0};
            emu::launch(blocks, 64, [&] { dir_head_kernel(&f, &dir, &info); }, 1);
            printf("H %d %u %u %u %u %u %u\n", e.status, e.aux, e.k, e.l, e.m, e.body_off, e.compressed);
        } else if (cmd == "text") {
            unsigned op; uint64_t off, n, src_at, dst_at, out_cap;
            in >> op >> off >> n >> src_at >> dst_at >> out_cap;
            if (off + n > blob.size()) return 3;
            Exact src(blob.data() + off, n, src_at);
            Guarded dst(out_cap, dst_at);
            const uint64_t tiles = text_tiles(n);
            std::vector<uint32_t> counts(tiles + 1, 0xEEEEEEEEu), firsts(tiles + 1, 0xEEEEEEEEu);
            std::vector<uint64_t> offs(tiles + 1, 0xEEEEEEEEEEEEEEEEull);
            TextJob job;
            memset(&job, 0, sizeof job);
            job.in = src.p; job.out = dst.p; job.len = n; job.out_cap = out_cap; job.tiles = tiles; job.op = (uint8_t)op;
            job.counts = counts.data(); job.firsts = firsts.data(); job.offs = offs.data();
            spng_result r;
            memset(&r, 0xEE, sizeof r);
            if (tiles) emu::launch(blocks, TEXT_THREADS, [&] { text_count_kernel(&job); }, 1);
            emu::launch(1, TEXT_THREADS, [&] { text_scan_kernel(&job, &r); });
            if (tiles && op == SPNG_TEXT_LATIN1_TO_UTF8) emu::launch(blocks, TEXT_THREADS, [&] { text_write_kernel(&job, &r); }, 1);
            bool ok = dst.intact() && counts[tiles] == 0xEEEEEEEEu && firsts[tiles] == 0xEEEEEEEEu && offs[tiles] == 0xEEEEEEEEEEEEEEEEull;
            if (!(r.status == SPNG_DONE && op == SPNG_TEXT_LATIN1_TO_UTF8))
                for (uint64_t i = 0; i < out_cap; ++i) ok = ok && dst.p[i] == 0xA5;        // nothing written
            else for (uint64_t i = r.written; i < out_cap; ++i) ok = ok && dst.p[i] == 0xA5;
            printf("T %d %llu %llu %llu %llu %d\n", r.status, (unsigned long long)r.written, (unsigned long long)r.consumed, (unsigned long long)r.aux[0],
                   (unsigned long long)r.aux[1], ok ? 1 : 0);
            if (r.status == SPNG_DONE && op == SPNG_TEXT_LATIN1_TO_UTF8) out_file.write((const char *)dst.p, (std::streamsize)r.written);
        } else if (!cmd.empty()) return 2;
    }
    return 0;
}
