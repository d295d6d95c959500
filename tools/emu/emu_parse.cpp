// emu_parse.cpp -- TEST INFRASTRUCTURE: runs the kernels of the typed chunks (csrc/chunks.hip: parse_scope -> parse_value -> parse_first,
// behind lex_walk -> lex_chunk -> lex_finish -> dir_list -> dir_head) on the CPU (tools/emu/hip/hip_runtime.h), from a prepared copy of
// the source as written (EMU_CHUNKS_SRC: launches blanked).  It prints what the kernels answer; the yardstick is the test's
// (tests/parse_ref.py).  Built and used by tests/test_emu_parse.py, never part of the product.  Every buffer the kernels see -- the
// file, the entries, the records, the infos, the summary -- sits between the guard bytes of guard.hpp, or, in a build with the address
// sanitizer, is exactly its bytes on the heap.
//
//   emu_parse <blob file> <script file>
// script, a command per line (offsets and lengths are into the blob file):
//   blocks <n>                 workgroups along x of the per-entry kernels (default 3)
//   file <off> <len> <cap>     the file blob[off, off + len) through all eight kernels with a directory of `cap` entries
//   parse <off> <len> <cap>    the three parse kernels alone over a directory this driver writes by walking the chunk headers (a file that
//                              lexes cleanly: no checksum is looked at)
// both print
//   P status index aux0 aux1 ihdr_index plte_index palette_count depth color ios interlaced
//   V status scope aux0 aux1 count k v0 ... v7          per record in front of min(chunks, cap)
//   G untouched                1: the records behind them are as they were, and so is every guard byte
#include EMU_CHUNKS_SRC

#include "guard.hpp"

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

static uint32_t word(const uint8_t *p) { return (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | p[3]; }

int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    const std::vector<uint8_t> blob = slurp(argv[1]);
    std::ifstream script(argv[2]);
    uint32_t blocks = 3;
    std::string line;
    while (std::getline(script, line)) {
        std::istringstream in(line);
        std::string cmd;
        in >> cmd;
        if (cmd == "blocks") { in >> blocks; continue; }
        if (cmd.empty()) continue;
        if (cmd != "file" && cmd != "parse") return 2;
        uint64_t off, n, cap;
        in >> off >> n >> cap;
        if (off + n > blob.size()) return 3;
        emu::Guarded file(std::vector<uint8_t>(blob.begin() + off, blob.begin() + off + n));
        emu::Guarded ent((cap + 2) * sizeof(spng_chunk_entry)), val((cap + 2) * sizeof(spng_chunk_value));
        emu::Guarded lexed(sizeof(spng_lexed)), summary(sizeof(spng_parsed)), desc(sizeof(spng_file_desc)), dirs(sizeof(spng_chunk_dir));
        emu::Guarded vptr(sizeof(spng_chunk_value *));
        spng_lexed &info = *(spng_lexed *)lexed.data();
        memset(&info, 0, sizeof info);
        std::vector<uint8_t> idat(n ? n : 1, 0xEE);
        spng_file_desc &f = *(spng_file_desc *)desc.data();
        f = spng_file_desc{file.data(), n, idat.data(), n};
        spng_chunk_dir &dir = *(spng_chunk_dir *)dirs.data();
        dir = spng_chunk_dir{cap ? (spng_chunk_entry *)ent.data() : nullptr, (uint32_t)cap, 0};
        spng_chunk_value *&values = *(spng_chunk_value **)vptr.data();
        values = cap ? (spng_chunk_value *)val.data() : nullptr;
        if (cmd == "file") {
            const uint64_t listed = lex_listed(n);
            uint64_t table_at[2] = {0, listed};
            std::vector<LexChunk> table(listed + 1);
            LexWalk walk;
            emu::launch(1, 64, [&] { lex_walk_kernel(&f, &info, table.data(), table_at, &walk); });
            emu::launch(blocks, 64, [&] { lex_chunk_kernel(&f, table.data(), table_at, &walk); }, 1);
            emu::launch(1, 64, [&] { lex_finish_kernel(&info, table.data(), table_at, &walk, &f, 1); });
            emu::launch(1, 64, [&] { dir_list_kernel(&f, &dir, &info, table.data(), table_at, &walk); });
            emu::launch(blocks, 64, [&] { dir_head_kernel(&f, &dir, &info); }, 1);
        } else {
            spng_chunk_entry *e = (spng_chunk_entry *)ent.data();
            uint64_t at = 8;
            while (at + 12 <= n) {
                const uint32_t length = word(file.data() + at), type = word(file.data() + at + 4);
                if (info.chunks < cap) {
                    spng_chunk_entry &x = e[info.chunks];
                    memset(&x, 0, sizeof x);
                    x.type = type; x.length = length; x.offset = at + 8; x.k = x.l = x.m = SPNG_NO_OFFSET;
                }
                info.chunks += 1;
                at += 12 + (uint64_t)length;
                if (type == 0x49454e44) break;
            }
            if (at > n) return 3;
        }
        const uint64_t filled = info.chunks < cap ? info.chunks : cap;
        emu::launch(1, 64, [&] { parse_scope_kernel(&f, &dir, &info, &values, (spng_parsed *)summary.data()); });
        emu::launch(blocks, 64, [&] { parse_value_kernel(&f, &dir, &info, &values, (const spng_parsed *)summary.data()); }, 1);
        emu::launch(1, 64, [&] { parse_first_kernel(&dir, &info, &values, (spng_parsed *)summary.data()); });
        const spng_parsed &p = *(const spng_parsed *)summary.data();
        printf("P %d %u %llu %llu %u %u %u %u %u %u %u\n", p.status, p.index, (unsigned long long)p.aux[0], (unsigned long long)p.aux[1], p.ihdr_index,
               p.plte_index, p.palette_count, p.depth, p.color, p.ios, p.interlaced);
        const spng_chunk_value *v = (const spng_chunk_value *)val.data();
        for (uint64_t i = 0; i < filled; ++i) {
            printf("V %d %u %llu %llu %u %u", v[i].status, v[i].scope, (unsigned long long)v[i].aux[0], (unsigned long long)v[i].aux[1], v[i].count, v[i].k);
            for (uint32_t w : v[i].v) printf(" %u", w);
            printf("\n");
        }
        bool untouched = file.intact("file") && ent.intact("entries") && val.intact("values") && lexed.intact("infos") && summary.intact("parsed") &&
                         desc.intact("file desc") && dirs.intact("dir") && vptr.intact("value pointers");
        for (size_t i = filled * sizeof(spng_chunk_value); i < val.size(); ++i) untouched = untouched && val.data()[i] == 0xEE;
        for (size_t i = filled * sizeof(spng_chunk_entry); i < ent.size(); ++i) untouched = untouched && ent.data()[i] == 0xEE;
        printf("G %d\n", untouched ? 1 : 0);
    }
    return 0;
}
