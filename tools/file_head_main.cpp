// file_head_main.cpp -- TEST INFRASTRUCTURE: a stand-alone program around csrc/file_head.hpp, the host code that lays down the head of
// a PNG file.  Built by tests/test_file_head.py with g++, plain and with -fsanitize=address,undefined, and run as a subprocess; the
// yardstick is the test's (tests/file_ref.py).  Never part of the product.
//
//   file_head_main <case file> <heads out file>
// a case per line, numbers in decimal:
//   width height depth channels indexed bgr interlaced chunk_bytes  has_key k0 k1 k2  has_fill f0 f1 f2
//   palette_count {r g b a}...  before_count {type len seed}...  after_count {type len seed}...
// (byte i of a blob is (seed + 7 i + (i >> 8)) & 255, held in an allocation of exactly its length).  Prints per case
//   status head_len bound
// -- bound: file_bound for a stream of 100 000 bytes -- and appends the head to the out file.
#include "../swift_png_amd/csrc/file_head.hpp"

#include <fstream>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>

using namespace spng;

int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    std::ifstream cases(argv[1]);
    std::ofstream out(argv[2], std::ios::binary);
    std::string line;
    while (std::getline(cases, line)) {
        if (line.empty()) continue;
        std::istringstream in(line);
        spng_png_desc d;
        memset(&d, 0, sizeof d);
        unsigned v[8];
        unsigned long long chunk_bytes;
        in >> d.width >> d.height;
        for (int k = 0; k < 5; ++k) in >> v[k];
        d.depth = (uint8_t)v[0]; d.channels = (uint8_t)v[1]; d.indexed = (uint8_t)v[2]; d.bgr = (uint8_t)v[3]; d.interlaced = (uint8_t)v[4];
        in >> chunk_bytes;
        d.chunk_bytes = chunk_bytes;
        in >> v[0] >> d.key[0] >> d.key[1] >> d.key[2] >> v[1] >> d.fill[0] >> d.fill[1] >> d.fill[2];
        d.has_key = (uint8_t)v[0]; d.has_fill = (uint8_t)v[1];
        in >> d.palette_count;
        std::unique_ptr<uint8_t[]> palette(new uint8_t[4 * (size_t)d.palette_count]);     // (exactly its length: a read behind it is seen)
        for (size_t k = 0; k < 4 * (size_t)d.palette_count; ++k) { in >> v[0]; palette[k] = (uint8_t)v[0]; }
        d.palette = d.palette_count ? palette.get() : nullptr;
        std::vector<spng_blob> blobs[2];
        std::vector<std::unique_ptr<uint8_t[]>> store;
        for (int g = 0; g < 2; ++g) {
            unsigned count;
            in >> count;
            for (unsigned b = 0; b < count; ++b) {
                spng_blob blob;
                unsigned seed;
                in >> blob.type >> blob.len >> seed;
                store.emplace_back(new uint8_t[blob.len]);
                for (uint32_t i = 0; i < blob.len; ++i) store.back()[i] = (uint8_t)(seed + 7 * i + (i >> 8));
                blob.data = blob.len ? store.back().get() : nullptr;
                blobs[g].push_back(blob);
            }
        }
        if (!in) return 3;
        d.before = blobs[0].data(); d.before_count = (uint32_t)blobs[0].size();
        d.after = blobs[1].data(); d.after_count = (uint32_t)blobs[1].size();
        std::vector<uint8_t> head;
        const int32_t status = file_head(d, head);
        if (status != SPNG_DONE && !head.empty()) return 4;    // (a refusal appends nothing)
        printf("%d %zu %llu\n", status, head.size(), (unsigned long long)file_bound(d, 100000));
        out.write((const char *)head.data(), (std::streamsize)head.size());
    }
    return 0;
}
