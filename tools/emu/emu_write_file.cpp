// emu_write_file.cpp -- TEST INFRASTRUCTURE: runs the file writer of csrc/chunks.hip (wfile_body_kernel -> wfile_finish_kernel) on the CPU
// (tools/emu/hip/hip_runtime.h), from a prepared copy of the source (EMU_WRITE_FILE_SRC: launches blanked).  It prints what the kernels
// answer and writes the files; the yardstick is the test's (tests/file_ref.py).  Built and used by tests/test_emu_write_file.py, never part
// of the product.  Every buffer the kernels see is an allocation that ENDS where the buffer ends and starts `residue` bytes in front of
// it (malloc aligns to 16, so the buffer's address has that residue mod 16), the bytes in front filled with a guard pattern that is looked
// at afterwards: a sanitizer build sees an access behind a buffer, the guards a write in front of it.
//
//   emu_write_file <script file> <blob file> <out file>
// script, a command per line, numbers in decimal:
//   file <head_off> <head_len> <head_res> <stream_off> <stream_alloc> <stream_res> <len> <stream_cap> <chunk_bytes> <out_alloc> <out_res>
//        <out_cap> <src> <src_status> <src_written> <src_aux0> <src_aux1>
//       a file of the next batch: head and stream are bytes of the blob file (stream_alloc of them are the stream's buffer); src 0: the
//       length is `len`, a host value; src 1: it is read from a spng_result {src_status, written, aux} in "device" memory
//   run <blocks_x>
//       the batch as one launch, blocks_x workgroups per file (0: file_blocks_x of the batch, as the host layer has it).  Prints per file
//           status written consumed aux0 aux1 clean
//       (clean: every guard is intact, and of the output buffer everything behind `written` -- all of it unless the status is SPNG_DONE --
//       still holds its fill) and appends the file's bytes (SPNG_DONE only) to the out file
#include EMU_WRITE_FILE_SRC
#include "geometry.hpp"

#include <fstream>
#include <iostream>
#include <sstream>
#include <vector>

using namespace spng;

struct Guarded {
    uint8_t *base = nullptr, *p = nullptr;
    uint64_t res = 0, len = 0;
    void make(uint64_t residue, uint64_t n, uint8_t fill)
    {
        res = residue & 15; len = n;
        base = (uint8_t *)malloc(res + n ? res + n : 1);
        if ((uint64_t)base & 15) abort();
        p = base + res;
        memset(base, 0xA5, res);
        memset(p, fill, n);
    }
    bool intact() const { for (uint64_t i = 0; i < res; ++i) if (base[i] != 0xA5) return false; return true; }
    void drop() { free(base); base = p = nullptr; }
};

struct File { Guarded head, stream, out, src, partial; FileJob job; };

int main(int argc, char **argv)
{
    if (argc < 4) return 2;
    std::ifstream script(argv[1]);
    std::ifstream bf(argv[2], std::ios::binary);
    const std::vector<uint8_t> blob((std::istreambuf_iterator<char>(bf)), std::istreambuf_iterator<char>());
    std::ofstream files_out(argv[3], std::ios::binary);
    std::vector<File> batch;
    uint64_t most_units = 1, finish_chunks = 0;
    std::string line;
    while (std::getline(script, line)) {
        std::istringstream in(line);
        std::string cmd;
        in >> cmd;
        if (cmd == "file") {
            uint64_t head_off, head_len, head_res, stream_off, stream_alloc, stream_res, len, stream_cap, chunk_bytes, out_alloc, out_res, out_cap;
            uint64_t src, src_written, src_aux0, src_aux1;
            int64_t src_status;
            in >> head_off >> head_len >> head_res >> stream_off >> stream_alloc >> stream_res >> len >> stream_cap >> chunk_bytes >> out_alloc >>
                out_res >> out_cap >> src >> src_status >> src_written >> src_aux0 >> src_aux1;
            if (!in || head_off + head_len > blob.size() || stream_off + stream_alloc > blob.size()) return 3;
            batch.emplace_back();
            File &f = batch.back();
            f.head.make(head_res, head_len, 0); memcpy(f.head.p, blob.data() + head_off, head_len);
            f.stream.make(stream_res, stream_alloc, 0); memcpy(f.stream.p, blob.data() + stream_off, stream_alloc);
            f.out.make(out_res, out_alloc, 0xEE);
            f.src.make(8, sizeof(spng_result), 0);
            spng_result sr{(int32_t)src_status, 0, src_written, 0, {src_aux0, src_aux1}};
            memcpy(f.src.p, &sr, sizeof sr);
            // the scratch for raw sums, sized as the host layer sizes it: a word per unit the capacity allows
            const uint64_t units = file_units(stream_cap, chunk_bytes);
            const bool folds = chunk_bytes > FILE_PIECE_BYTES && stream_cap > FILE_PIECE_BYTES;
            f.partial.make(0, folds ? 4 * units : 0, 0xCD);
            most_units = units > most_units ? units : most_units;
            if (folds) finish_chunks = std::max(finish_chunks, file_chunks(stream_cap, chunk_bytes));
            FileJob &j = f.job;
            memset(&j, 0, sizeof j);
            j.head = f.head.p; j.head_len = head_len; j.stream = f.stream.p; j.src_result = src ? (const spng_result *)f.src.p : nullptr;
            j.len = src ? 0 : len; j.stream_cap = stream_cap; j.out = f.out.p; j.out_cap = out_cap; j.chunk_bytes = chunk_bytes;
            j.partial = folds ? (uint32_t *)f.partial.p : nullptr;
        } else if (cmd == "run") {
            uint64_t bx;
            in >> bx;
            const uint32_t count = (uint32_t)batch.size();
            if (!count) return 3;
            if (!bx) bx = file_blocks_x(count, most_units);
            std::vector<FileJob> jobs(count);
            for (uint32_t i = 0; i < count; ++i) jobs[i] = batch[i].job;
            std::vector<spng_result> results(count);
            memset(results.data(), 0x77, count * sizeof(spng_result));
            emu::launch((unsigned)bx, 64, [&] { wfile_body_kernel(jobs.data(), results.data()); }, count);
            if (finish_chunks) {
                const unsigned fx = (unsigned)std::min<uint64_t>((finish_chunks + 63) / 64, 1024);
                emu::launch(fx, 64, [&] { wfile_finish_kernel(jobs.data(), results.data()); }, count);
            }
            for (uint32_t i = 0; i < count; ++i) {
                File &f = batch[i];
                const spng_result &r = results[i];
                const uint64_t kept = r.status == SPNG_DONE ? r.written : 0;
                if (kept > f.out.len) return 4;
                bool clean = f.head.intact() && f.stream.intact() && f.out.intact() && f.src.intact() && r.reserved == 0;
                for (uint64_t k = kept; k < f.out.len; ++k) clean = clean && f.out.p[k] == 0xEE;
                printf("%d %llu %llu %llu %llu %d\n", r.status, (unsigned long long)r.written, (unsigned long long)r.consumed,
                       (unsigned long long)r.aux[0], (unsigned long long)r.aux[1], clean ? 1 : 0);
                files_out.write((const char *)f.out.p, (std::streamsize)kept);
                f.head.drop(); f.stream.drop(); f.out.drop(); f.src.drop(); f.partial.drop();
            }
            batch.clear(); most_units = 1; finish_chunks = 0;
        } else if (!cmd.empty()) return 2;
    }
    return 0;
}
