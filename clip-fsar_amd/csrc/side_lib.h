// Host error plumbing of the side libraries (gallery.hip, gallery_text.hip, stream.hip, pool.hip, ingest.hip, live.hip, groups.hip, lastblock.hip, enroll.hip, live_text.hip;
// through otam_tile.h for gallery.hip, live.hip, groups.hip and live_text.hip): each is ONE translation unit, so these are internal-linkage items -- every library gets its own thread-local
// message buffer and exports nothing of it.  (libclipfsar_hip.so shares cfsar_fail etc. across its translation units by linkage
// instead: runtime.hip, which is not linked into the side libraries.)
#pragma once
#include <stdarg.h>
#include <stdint.h>
#include <stdlib.h>

#include "common.h"

namespace {

thread_local char g_err[512] = {0};

int fail(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return 1;
}

int check_launch(const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail("%s: %s", what, hipGetErrorString(e));
    return 0;
}

// One bit per slot of [0, cap), on the heap: the "slot appears twice" scan of a descriptor table's host rows (pool.hip, live.hip)
struct SlotBits {
    uint64_t* words;
    explicit SlotBits(int cap) : words(static_cast<uint64_t*>(calloc(((size_t)cap + 63) / 64, sizeof(uint64_t)))) {}
    SlotBits(const SlotBits&) = delete;
    ~SlotBits() { free(words); }
    bool ok() const { return words != nullptr; }
    bool test_and_set(int slot) {                      // was the slot's bit set already?
        const uint64_t bit = (uint64_t)1 << (slot & 63);
        const bool was = words[slot >> 6] & bit;
        words[slot >> 6] |= bit;
        return was;
    }
};

}  // namespace

#define SIDE_REQUIRE(cond, ...)               \
    do {                                      \
        if (!(cond)) return fail(__VA_ARGS__); \
    } while (0)
