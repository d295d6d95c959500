// emu_gzip.cpp -- TEST INFRASTRUCTURE: runs the kernels of csrc/gzip.hip on the CPU (tools/emu/hip/hip_runtime.h): the header parser, the
// CRC-32 in 256 pieces with its fold, the Adler-32 of a stream that arrived in pieces, and the trailer writer.  From a prepared copy of the
// source (EMU_GZIP_SRC: launches blanked); built and used by tests/test_emu_gzip.py, never part of the product.  Every source and
// destination is a heap buffer of exactly its bytes, so that a build with the address sanitizer sees a read behind src_len and a write
// behind dst_cap.
//
//   emu_gzip pre <file of concatenated sources> <file of their lengths, one per line>
//       gzip_pre_kernel over all of them in one launch.  A line per source:
//       status aux0 gz job_off job_len job_format stream_off stream_len stream_format done
//       (status: the result's where `done` was set, else 0; gz: the payload offset, or -1; *_off: how far the window moved)
//   emu_gzip crc <file>                     gzip_deflate_crc_kernel + fold_pieces: prints the CRC-32 (hex)
//   emu_gzip adler <file> <declared (hex)>  resume_adler_kernel + resume_post_kernel over the file as the output of a finished stream whose
//                                           trailer declares that sum: prints status aux0 aux1 (hex)
//   emu_gzip trailer <file> <body bytes>    gzip_deflate_post_kernel behind a stream of <body bytes>, dst_cap = body + 0 ... body + 8: a line per
//                                           capacity: status written <the bytes stored behind the body (hex, or -)>
#include EMU_GZIP_SRC

#include <fstream>
#include <iostream>
#include <string>
#include <vector>

using namespace spng;

static std::vector<uint8_t> slurp(const char *path)
{
    std::ifstream f(path, std::ios::binary);
    return std::vector<uint8_t>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}
static uint8_t *exact(const uint8_t *p, size_t n)
{
    uint8_t *q = (uint8_t *)malloc(n ? n : 1);
    if (n) memcpy(q, p, n);
    return q;
}

int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    const std::string mode = argv[1];
    const std::vector<uint8_t> file = slurp(argv[2]);
    if (mode == "pre" && argc >= 4) {
        std::ifstream lens(argv[3]);
        std::vector<uint64_t> len;
        for (uint64_t v; lens >> v;) len.push_back(v);
        const uint32_t count = (uint32_t)len.size();
        std::vector<InflateJob> jobs(count);
        std::vector<PStream> streams(count);
        std::vector<spng_result> results(count);
        std::vector<uint64_t> gz(count, 12345);
        std::vector<int32_t> done(count, 0);
        std::vector<uint8_t *> src(count);
        uint64_t at = 0;
        for (uint32_t i = 0; i < count; ++i) {
            if (at + len[i] > file.size()) return 3;
            src[i] = exact(file.data() + at, len[i]);
            at += len[i];
            memset(&jobs[i], 0, sizeof(InflateJob)); memset(&streams[i], 0, sizeof(PStream)); memset(&results[i], 0xff, sizeof(spng_result));
            jobs[i].src = streams[i].src = src[i]; jobs[i].src_len = streams[i].src_len = len[i];
            jobs[i].format = streams[i].format = SPNG_FORMAT_GZIP; jobs[i].image = streams[i].image = i;
        }
        if (at != file.size()) return 3;
        emu::launch((count + 63) / 64, 64, [&] { gzip_pre_kernel(jobs.data(), streams.data(), results.data(), gz.data(), done.data(), count); });
        for (uint32_t i = 0; i < count; ++i) {
            printf("%d %llu %lld %llu %llu %d %llu %llu %d %d\n", done[i] ? results[i].status : 0, done[i] ? (unsigned long long)results[i].aux[0] : 0ull,
                   (long long)gz[i], (unsigned long long)(jobs[i].src - src[i]), (unsigned long long)jobs[i].src_len, jobs[i].format,
                   (unsigned long long)(streams[i].src - src[i]), (unsigned long long)streams[i].src_len, streams[i].format, done[i]);
            free(src[i]);
        }
        return 0;
    }
    const uint64_t n = file.size();
    uint8_t *buf = exact(file.data(), n);
    if (mode == "crc") {
        DeflateJob job;
        memset(&job, 0, sizeof job);
        job.src = buf; job.src_len = n; job.format = SPNG_FORMAT_GZIP;
        std::vector<uint32_t> parts(GZ_PIECES, 0xDEADBEEF);
        uint32_t crc = 0;
        emu::launch(GZ_PIECES, 64, [&] { gzip_deflate_crc_kernel(&job, parts.data()); });
        emu::launch(1, 1, [&] { crc = fold_pieces(parts.data(), n); });
        printf("%08x\n", crc);
        return 0;
    }
    if (mode == "adler" && argc >= 4) {
        const uint32_t declared = (uint32_t)strtoul(argv[3], nullptr, 16);
        const uint8_t trailer[4] = {(uint8_t)(declared >> 24), (uint8_t)(declared >> 16), (uint8_t)(declared >> 8), (uint8_t)declared};
        uint8_t *t = exact(trailer, 4);
        uint64_t state[4] = {0, 0, 0, 0};
        InflateJob job;
        memset(&job, 0, sizeof job);
        job.src = t; job.src_len = 4; job.dst = buf; job.dst_cap = n; job.format = SPNG_FORMAT_ZLIB; job.state = state;
        spng_result res;
        memset(&res, 0, sizeof res);
        res.status = SPNG_DONE; res.written = n; res.consumed = 4;
        std::vector<uint64_t> parts(GZ_PIECES, ~0ull);
        emu::launch(GZ_PIECES, 64, [&] { resume_adler_kernel(&job, &res, parts.data()); });
        emu::launch(1, 64, [&] { resume_post_kernel(&job, &res, parts.data(), 1); });
        printf("%d %llx %llx\n", res.status, (unsigned long long)res.aux[0], (unsigned long long)res.aux[1]);
        return 0;
    }
    if (mode == "trailer" && argc >= 4) {
        const uint64_t body = strtoull(argv[3], nullptr, 10);
        DeflateJob job;
        memset(&job, 0, sizeof job);
        job.src = buf; job.src_len = n; job.format = SPNG_FORMAT_GZIP;
        std::vector<uint32_t> parts(GZ_PIECES, 0xDEADBEEF);
        emu::launch(GZ_PIECES, 64, [&] { gzip_deflate_crc_kernel(&job, parts.data()); });
        for (uint64_t c = 0; c <= 8; ++c) {
            uint8_t *dst = (uint8_t *)malloc(body + c ? body + c : 1);
            memset(dst, 0xEE, body + c);
            job.dst = dst; job.dst_cap = body + c;
            spng_result res;
            memset(&res, 0, sizeof res);
            res.status = SPNG_DONE; res.written = body; res.consumed = n;
            emu::launch(1, 64, [&] { gzip_deflate_post_kernel(&job, &res, parts.data(), 1); });
            printf("%d %llu ", res.status, (unsigned long long)res.written);
            for (uint64_t k = 0; k < c; ++k) printf("%02x", dst[body + k]);
            bool kept = true;
            for (uint64_t k = 0; k < body; ++k) kept = kept && dst[k] == 0xEE;
            printf("%s%s\n", c ? "" : "-", kept ? "" : " BODY-CHANGED");
            free(dst);
        }
        return 0;
    }
    return 2;
}
