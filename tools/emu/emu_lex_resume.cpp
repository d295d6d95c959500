// emu_lex_resume.cpp -- TEST INFRASTRUCTURE: runs the chunk lexers of csrc/chunks.hip on the CPU (tools/emu/hip/hip_runtime.h): the
// resumable one (lexr_walk -> lexr_piece -> lexr_finish) over a file that arrives push by push, and the whole-file one (lex_walk ->
// lex_chunk -> lex_finish) over prefixes as whole files.  It prints what the kernels answer and writes the IDAT bytes; the yardstick is the test's
// (tests/lex_ref.py).  From a prepared copy of the source (EMU_LEX_RESUME_SRC: launches blanked); built and used by
// tests/test_emu_lex_resume.py, never part of the product.  Every run hands the kernels a fresh copy of exactly the prefix and an IDAT
// buffer of exactly its capacity, so that a sanitizer build sees a read behind the bytes that have arrived and a write behind idat_cap.
//
//   emu_lex_resume <png file> <script file> <idat out file>
// script, a command per line:
//   reset                 a zero-filled state, an untouched IDAT buffer, counters cleared
//   cap <bytes>           idat_cap from now on (default: the file's length)
//   list <entries>        capacity of the list (default: lex_resume_listed / lex_listed of the prefix; 0 is allowed: everything overflows)
//   waves <n>             waves of the piece / chunk kernel (default 3)
//   poke <offset> <byte>  overwrites a byte of the state
//   flip <offset> <mask>  xors a byte of the file (from now on)
//   nostate               the next push gets a null state
//   push <len>            lexes the first len bytes with the state.  Prints
//       status chunks aux0 aux1 width height depth color compression filter interlace ios idat_len plte_off plte_len trns_off trns_len consumed pad0 pad1 summed copied headers
//     (summed / copied / headers: this push's counters) and appends the IDAT bytes in front of idat_len to the out file
//   whole <len>           the same for the first len bytes as a whole file: no state, a fresh IDAT buffer, counters 0
//   total                 prints the counters summed since the last reset: summed copied headers pushes
#include EMU_LEX_RESUME_SRC
#include "geometry.hpp"

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

int main(int argc, char **argv)
{
    if (argc < 4) return 2;
    std::vector<uint8_t> png = slurp(argv[1]);
    std::ifstream script(argv[2]);
    std::ofstream idat_out(argv[3], std::ios::binary);
    const uint64_t total = png.size();
    uint64_t cap = total;
    int64_t list_cap = -1;
    uint32_t waves = 3;
    bool nostate = false;
    std::vector<uint8_t> state(sizeof(LexState), 0), idat(total ? total : 1, 0xEE);
    unsigned long long sums[4] = {0, 0, 0, 0};
    std::string line;
    while (std::getline(script, line)) {
        std::istringstream in(line);
        std::string cmd;
        in >> cmd;
        if (cmd == "reset") {
            std::fill(state.begin(), state.end(), 0); std::fill(idat.begin(), idat.end(), 0xEE);
            sums[0] = sums[1] = sums[2] = sums[3] = 0;
        } else if (cmd == "cap") in >> cap;
        else if (cmd == "list") in >> list_cap;
        else if (cmd == "waves") in >> waves;
        else if (cmd == "nostate") nostate = true;
        else if (cmd == "poke") { uint64_t at; unsigned v; in >> at >> v; if (at < state.size()) state[at] = (uint8_t)v; }
        else if (cmd == "flip") { uint64_t at; unsigned v; in >> at >> v; if (at < total) png[at] ^= (uint8_t)v; }
        else if (cmd == "total") printf("%llu %llu %llu %llu\n", sums[0], sums[1], sums[2], sums[3]);
        else if (cmd == "push" || cmd == "whole") {
            const bool resumed = cmd == "push";
            uint64_t n;
            in >> n;
            if (n > total) return 3;
            // exactly the prefix, and an IDAT buffer of exactly its capacity
            uint8_t *prefix = (uint8_t *)malloc(n ? n : 1), *dst = (uint8_t *)malloc(cap ? cap : 1);
            memcpy(prefix, png.data(), n);
            if (resumed) memcpy(dst, idat.data(), cap < idat.size() ? cap : idat.size());
            else memset(dst, 0xEE, cap ? cap : 1);
            spng_file_desc f{prefix, n, dst, cap};
            void *sp = nostate ? nullptr : state.data();
            if (resumed) nostate = false;
            spng_lexed out;
            memset(&out, 0, sizeof out);
            const uint64_t listed = list_cap >= 0 ? (uint64_t)list_cap : resumed ? lex_resume_listed(n) : lex_listed(n);
            uint64_t table_at[2] = {0, listed};
            unsigned long long stats[3] = {0, 0, 0};
            if (resumed) {
                std::vector<LexPiece> table(listed + 1);
                LexRWalk walk;
                emu::launch(1, 64, [&] { lexr_walk_kernel(&f, &sp, &out, table.data(), table_at, &walk); });
                emu::launch(waves, 64, [&] { lexr_piece_kernel(&f, table.data(), table_at, &walk); }, 1);
                emu::launch(1, 64, [&] { lexr_finish_kernel(&out, table.data(), table_at, &walk, &f, &sp, stats, 1); });
                memcpy(idat.data(), dst, cap < idat.size() ? cap : idat.size());
                for (int k = 0; k < 3; ++k) sums[k] += stats[k];
                sums[3] += 1;
            } else {
                std::vector<LexChunk> table(listed + 1);
                LexWalk walk;
                emu::launch(1, 64, [&] { lex_walk_kernel(&f, &out, table.data(), table_at, &walk); });
                emu::launch(waves, 64, [&] { lex_chunk_kernel(&f, table.data(), table_at, &walk); }, 1);
                emu::launch(1, 64, [&] { lex_finish_kernel(&out, table.data(), table_at, &walk, &f, 1); });
            }
            if (out.idat_len > cap) return 4;
            idat_out.write((const char *)dst, (std::streamsize)out.idat_len);
            free(prefix); free(dst);
            printf("%d %u %llx %llx %u %u %u %u %u %u %u %u %llu %llu %u %llu %u %llu %u %u %llu %llu %llu\n", out.status, out.chunks, (unsigned long long)out.aux[0],
                   (unsigned long long)out.aux[1], out.width, out.height, out.depth, out.color, out.compression, out.filter, out.interlace, out.ios,
                   (unsigned long long)out.idat_len, (unsigned long long)out.plte_off, out.plte_len, (unsigned long long)out.trns_off, out.trns_len,
                   (unsigned long long)out.consumed, out.pad[0], out.pad[1], stats[0], stats[1], stats[2]);
        } else if (!cmd.empty()) return 2;
    }
    return 0;
}
