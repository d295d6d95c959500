// guard.hpp -- TEST INFRASTRUCTURE: the source and destination buffers of the emulator drivers.
//
// A plain build puts GUARD bytes of 0xEE on both sides of a buffer and looks at them after the kernels ran: a changed byte is a
// write outside the buffer, named by its offset (exit code EXIT_GUARD of the driver).  A build with the address sanitizer gives the
// buffer exactly its bytes on the heap, nothing around them: there the sanitizer reports the access itself -- reads behind a source's
// end included, which guard bytes cannot see.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#if defined(__SANITIZE_ADDRESS__)
#define EMU_EXACT_BUFFERS 1
#elif defined(__has_feature)
#if __has_feature(address_sanitizer)
#define EMU_EXACT_BUFFERS 1
#endif
#endif

namespace emu {

static constexpr int EXIT_GUARD = 6;

struct Guarded {
#ifdef EMU_EXACT_BUFFERS
    static constexpr size_t GUARD = 0;
#else
    static constexpr size_t GUARD = 64;
#endif
    uint8_t *base;
    size_t n;
    explicit Guarded(size_t bytes) : base(new uint8_t[bytes + 2 * GUARD]), n(bytes) { memset(base, 0xEE, bytes + 2 * GUARD); }
    explicit Guarded(const std::vector<uint8_t> &content) : Guarded(content.size()) { if (n) memcpy(data(), content.data(), n); }
    Guarded(const Guarded &) = delete;
    ~Guarded() { delete[] base; }
    uint8_t *data() const { return base + GUARD; }
    size_t size() const { return n; }
    // every guard byte as it was?  The first changed one is printed: its offset from the buffer's first byte
    bool intact(const char *what) const
    {
        for (size_t i = 0; i < GUARD; ++i)
            if (base[GUARD - 1 - i] != 0xEE) { printf("%s: guard byte changed %zu in front of the buffer\n", what, i + 1); return false; }
        for (size_t i = 0; i < GUARD; ++i)
            if (base[GUARD + n + i] != 0xEE) { printf("%s: guard byte changed at offset %zu, %zu behind the buffer's %zu bytes\n", what, n + i, i, n); return false; }
        return true;
    }
};

}  // namespace emu
