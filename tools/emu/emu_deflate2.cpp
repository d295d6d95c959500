// emu_deflate2.cpp -- TEST INFRASTRUCTURE: runs the round kernels of csrc/deflate.hip (dfl2_begin / dfl3_search /
// dfl2_advance / dfl2_parse) on the CPU (tools/emu/hip/hip_runtime.h) over one stream, round by round and with the two sets
// of candidate records alternating the way host_encode.hip drives them, and compares the bytes with the expected stream (the oracle's).
// Built and used by tests/test_emu_deflate.py from a copy of deflate.hip whose launchers and `s_waitcnt` lines are blanked
// (EMU_DEFLATE_SRC); never part of the product.
//
//   emu_deflate2 <input file> <expected stream file> <level> <format 0 zlib | 1 raw (ios)> [chunks per stream] [cut ...]
//   cut ...: the input arrives in pieces (spng_deflate_resume_batch): a call per cut with `more` set, the state kept, then the rest
//   EMU_EXPONENT=8...15: the window exponent (default 15, what PNG uses; the raw format always takes 15, DeflatorBuffers.swift:52-55)
//   EMU_DST_CAP=n: the output capacity (default: the expected stream's length + 4096).  Below that length the run succeeds exactly when
//   the status is SPNG_E_OUTPUT_CAPACITY, written is the expected stream's length and the first n bytes are the expected stream's; with
//   `cut ...` every push from the one that overflowed on must answer SPNG_E_OUTPUT_CAPACITY
//   The input has exactly its bytes and the output exactly its capacity, both between guard bytes (tools/emu/guard.hpp; under the
//   address sanitizer: exact heap buffers): exit code 6 when a guard byte changed (printed: which), whatever else happened
//   exit code 0: SPNG_DONE and identical bytes (or the capacity answer above); 1: anything else (printed)
#include EMU_DEFLATE_SRC
#include "guard.hpp"

#include <fstream>
#include <iostream>

using namespace spng;

static std::vector<uint8_t> slurp(const char *path)
{
    std::ifstream f(path, std::ios::binary);
    return std::vector<uint8_t>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

static int run(int argc, char **argv, const emu::Guarded &src, const std::vector<uint8_t> &want, emu::Guarded &dst);

int main(int argc, char **argv)
{
    if (argc < 5) { fprintf(stderr, "usage\n"); return 2; }
    const emu::Guarded src(slurp(argv[1]));
    const std::vector<uint8_t> want = slurp(argv[2]);
    emu::Guarded dst(getenv("EMU_DST_CAP") ? strtoull(getenv("EMU_DST_CAP"), nullptr, 10) : want.size() + 4096);
    const int code = run(argc, argv, src, want, dst);
    if (!src.intact("source") || !dst.intact("destination")) return emu::EXIT_GUARD;
    return code;
}

// the end of a run: the whole stream, or -- a capacity below its length -- the capacity answer
static int verdict(const spng_result &res, const std::vector<uint8_t> &want, const emu::Guarded &dst, uint64_t n, uint32_t rounds, const char *form)
{
    const uint64_t cap = dst.size(), head = cap < want.size() ? cap : want.size();
    const int32_t expect = cap < want.size() ? SPNG_E_OUTPUT_CAPACITY : SPNG_DONE;
    if (res.status != expect) { printf("status %d where %d is expected (capacity %llu, stream %zu)\n", res.status, expect, (unsigned long long)cap, want.size()); return 1; }
    if (res.written != want.size() || res.consumed != n || memcmp(dst.data(), want.data(), head)) {
        size_t k = 0;
        while (k < head && dst.data()[k] == want[k]) ++k;
        printf("stream differs: %llu bytes against %zu expected, consumed %llu of %llu, first difference at %zu of the first %llu\n", (unsigned long long)res.written,
               want.size(), (unsigned long long)res.consumed, (unsigned long long)n, k, (unsigned long long)head);
        return 1;
    }
    printf("ok%s: %llu -> %llu bytes in %u rounds%s\n", expect ? " (capacity)" : "", (unsigned long long)n, (unsigned long long)res.written, rounds, form);
    return 0;
}

// a push that is not the last: more input wanted -- or, from the push that overflowed on, the capacity error
static bool push_answer(const spng_result &res, bool &overflowed, size_t call)
{
    if (res.status == SPNG_E_OUTPUT_CAPACITY) overflowed = true;
    if (res.status == (overflowed ? SPNG_E_OUTPUT_CAPACITY : SPNG_NEED_MORE_INPUT)) return true;
    printf("call %zu (more): status %d%s\n", call, res.status, overflowed ? " after the stream had overflowed" : "");
    return false;
}

static int run(int argc, char **argv, const emu::Guarded &src, const std::vector<uint8_t> &want, emu::Guarded &dst)
{
    const int level = atoi(argv[3]), format = atoi(argv[4]);
    const uint32_t cps = argc > 5 ? (uint32_t)atoi(argv[5]) : 3;
    const uint64_t n = src.size();
    const int asked = getenv("EMU_EXPONENT") ? atoi(getenv("EMU_EXPONENT")) : 15;
    if (asked < 8 || asked > 15) { fprintf(stderr, "EMU_EXPONENT: 8 ... 15\n"); return 2; }
    const uint32_t exponent = format == 1 ? 15u : (uint32_t)asked;
    bool overflowed = false;

    if (level < 8) {
        // levels 0-7 in rounds: dfl3_begin -> (dfl3_search_fast + dfl3_advance, dfl3_parse) per round, the two sets of answers
        // alternating; `cut ...`: a call per piece with `more` set and the state kept, as spng_deflate_resume_batch drives it
        const uint64_t RV = deflate3_round_positions();
        std::vector<uint32_t> match[2] = {std::vector<uint32_t>(RV + 64, 0xDEADBEEF), std::vector<uint32_t>(RV + 64, 0xBEEFDEAD)};
        std::vector<uint8_t> statebuf(deflate_state_bytes(), 0);
        D3Stream st;
        memset(&st, 0, sizeof st);
        st.src = src.data(); st.dst = dst.data(); st.src_len = n; st.dst_cap = dst.size();
        st.format = format == 1 ? SPNG_FORMAT_IOS : SPNG_FORMAT_ZLIB; st.level = level; st.image = 0; st.exponent = exponent;
        st.state = (D1State *)statebuf.data();
        st.match[0] = match[0].data(); st.match[1] = match[1].data();
        spng_result res;
        memset(&res, 0xff, sizeof res);
        const uint32_t chunk = (uint32_t)(((RV / cps + 63) / 64) * 64);
        std::vector<uint64_t> cuts;
        for (int a = 6; a < argc; ++a) cuts.push_back(strtoull(argv[a], nullptr, 10));
        cuts.push_back(n);
        // one-shot streams: the blocks side by side (dfl4_walk / dfl4_block / dfl4_scan / dfl4_place), as host_encode.hip drives them;
        // EMU_TWO_WAVE forces the two-wave parse (the form of streams that arrive in pieces)
        const bool blocks = cuts.size() == 1 && !getenv("EMU_TWO_WAVE");
        const uint32_t maxb = (uint32_t)deflate4_max_blocks(RV);
        std::vector<uint32_t> terms(RV + 64 + 4096, 0xABABABAB), bdesc(4 + 2 * (size_t)maxb, 0);
        std::vector<uint64_t> bbits(2 * (size_t)maxb, 0);
        std::vector<uint8_t> scratch(blocks ? (size_t)maxb * deflate4_block_bytes() + 64 : 64, 0xCD);
        if (blocks) { st.terms = terms.data(); st.bdesc = bdesc.data(); st.bbits = bbits.data(); st.scratch = scratch.data(); }
        uint32_t rounds = 0;
        uint64_t spos = 0;
        for (size_t call = 0; call < cuts.size(); ++call) {
            st.src_len = cuts[call] < n ? cuts[call] : n;
            st.more = call + 1 < cuts.size() ? 1 : 0;
            const uint64_t E = deflate3_end(st.src_len, st.more != 0), span = E > spos ? E - spos : 0;
            const uint32_t calls_rounds = span ? (uint32_t)((span + RV - 1) / RV) : 1;
            emu::launch(1, 256, [&] { dfl3_begin_kernel(&st, 1); });
            for (uint32_t r = 0; r < calls_rounds; ++r, ++rounds) {
                const uint32_t par = r & 1;
                emu::launch(cps, SPNG_D3_WAVES * 64, [&] { dfl3_search_fast_kernel(&st, cps, chunk, par); });
                emu::launch(1, 256, [&] { dfl3_advance_kernel(&st, 1); });
                if (blocks) {
                    emu::launch(1, 64, [&] { dfl4_walk_kernel(&st, par); });
                    if (getenv("EMU_DUMP_TERMS")) {
                        std::ofstream o(getenv("EMU_DUMP_TERMS"), std::ios::binary);
                        const uint32_t nbk = bdesc[0]; uint32_t tot = 0;
                        for (uint32_t k = 0; k < nbk; ++k) tot += bdesc[5 + 2 * k] & 0x7fffffffu;
                        o.write((const char *)&nbk, 4); o.write((const char *)bdesc.data(), 4 * (4 + 2 * (size_t)nbk));
                        o.write((const char *)&tot, 4); o.write((const char *)terms.data(), 4 * (size_t)tot);
                        const uint32_t nm = (uint32_t)(n + 1); o.write((const char *)&nm, 4); o.write((const char *)match[par].data(), 4 * (size_t)nm);
                    }
                    // (the product launches the worst case of blocks -- the host does not know their number -- and the idle ones return at
                    //  once; here only the ones the walk made, + 1 idle: a workgroup costs the emulator 64 fibers)
                    const uint32_t grid = bdesc[0] + 1 < maxb ? bdesc[0] + 1 : maxb;
                    emu::launch(grid, 64, [&] { dfl4_block_kernel(&st); });
                    emu::launch(1, 256, [&] { dfl4_scan_kernel(&st, maxb, &res); });
                    emu::launch(grid, 64, [&] { dfl4_place_kernel(&st, maxb); });
                } else emu::launch(1, 128, [&] { dfl3_parse_kernel(&st, &res, par); });
            }
            if (st.more && !push_answer(res, overflowed, call)) return 1;
            if (st.more) { if (res.aux[1] != st.state->spos) { printf("call %zu: aux[1] %llu != spos %llu\n", call, (unsigned long long)res.aux[1], (unsigned long long)st.state->spos); return 1; } spos = res.aux[1]; }
        }
        if (!st.state->done) { printf("status %d done %u after %u rounds\n", res.status, st.state->done, rounds); return 1; }
        return verdict(res, want, dst, n, rounds, blocks ? " (search + parse kernels, blocks side by side)" : " (search + parse kernels)");
    }
    const uint64_t V = deflate2_vertices(n), B = V / 64 + 2;
    std::vector<uint16_t> vinfo[2] = {std::vector<uint16_t>(V, 0xDEAD), std::vector<uint16_t>(V, 0xBEEF)};
    std::vector<uint64_t> bbase[2] = {std::vector<uint64_t>(B, 0), std::vector<uint64_t>(B, 0)};
    std::vector<uint32_t> bwords[2] = {std::vector<uint32_t>(B, 0), std::vector<uint32_t>(B, 0)};
    std::vector<uint64_t> emask(B, 0);
    std::vector<uint32_t> up(V + 2, 0), step(V + 2, 0);
    std::vector<uint8_t> pathb(V + 2, 0), litb(B, 0);
    const uint64_t pool_words = (n < (1u << 21) ? n : (1u << 21)) * 30 + 4096;
    std::vector<uint32_t> pool[2] = {std::vector<uint32_t>(pool_words, 0), std::vector<uint32_t>(pool_words, 0)};
    unsigned long long pool_next[2] = {0, 0};
    std::vector<uint32_t> rings((size_t)cps * SPNG_D3_WAVES * 30 * 64, 0);    // (the search workgroups' word scratch)
    D2State state;
    memset(&state, 0, sizeof state);
    D2Stream st;
    memset(&st, 0, sizeof st);
    st.src = src.data(); st.dst = dst.data(); st.src_len = n; st.dst_cap = dst.size();
    st.format = format == 1 ? SPNG_FORMAT_IOS : SPNG_FORMAT_ZLIB; st.level = level; st.image = 0; st.exponent = exponent; st.more = 0;
    st.state = &state;
    st.vinfo = vinfo[0].data(); st.bbase = bbase[0].data(); st.bwords = bwords[0].data(); st.emask = emask.data();
    st.vinfo2 = vinfo[1].data(); st.bbase2 = bbase[1].data(); st.bwords2 = bwords[1].data();
    st.up = up.data(); st.step = step.data(); st.pathb = pathb.data(); st.litb = litb.data();
    spng_result res;
    memset(&res, 0xff, sizeof res);

    uint64_t pos = 0; uint32_t lim = 2048;
    const uint32_t chunk = ((D2_RV / cps + 63) / 64) * 64;
    std::vector<uint64_t> cuts;
    for (int a = 6; a < argc; ++a) cuts.push_back(strtoull(argv[a], nullptr, 10));
    cuts.push_back(n);
    uint32_t rounds = 0;
    for (size_t call = 0; call < cuts.size(); ++call) {
        // one call of spng_deflate_resume_batch: the bytes so far, `more` unless they are all
        st.src_len = cuts[call] < n ? cuts[call] : n;
        st.more = call + 1 < cuts.size() ? 1 : 0;
        const uint32_t calls_rounds = deflate2_plan(st.src_len, st.more != 0, pos, lim);
        emu::launch(1, 256, [&] { dfl2_begin_kernel(&st, 1); });
        for (uint32_t r = 0; r < calls_rounds; ++r, ++rounds) {
            const uint32_t par = r & 1;
            pool_next[par] = 0;
            emu::launch(cps, SPNG_D3_WAVES * 64, [&] { dfl3_search_kernel(&st, cps, chunk, pool[par].data(), &pool_next[par], pool_words, rings.data(), par); });
            emu::launch(1, 256, [&] { dfl2_advance_kernel(&st, 1); });
            emu::launch(1, 64, [&] { dfl2_parse_kernel(&st, pool[par].data(), &res, par); });
            if (getenv("EMU_VERBOSE")) fprintf(stderr, "call %zu round %u: pos %llu limit %u total %llu fail %u done %u status %d\n", call, r, (unsigned long long)state.pos,
                                               state.limit, (unsigned long long)state.total, state.fail, state.done, res.status);
        }
        if (st.more && !push_answer(res, overflowed, call)) return 1;
    }
    if (getenv("EMU_DUMP")) { std::ofstream o(getenv("EMU_DUMP"), std::ios::binary); o.write((const char *)dst.data(), (std::streamsize)(res.written < dst.size() ? res.written : dst.size())); }
    if (!state.done || state.fail) { printf("status %d done %u fail %u after %u rounds\n", res.status, state.done, state.fail, rounds); return 1; }
    return verdict(res, want, dst, n, rounds, "");
}
