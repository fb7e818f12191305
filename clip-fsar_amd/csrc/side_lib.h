// Host error plumbing of the side libraries (gallery.hip, gallery_text.hip, stream.hip, pool.hip): each is ONE translation unit, so these are internal-linkage
// items -- every library gets its own thread-local message buffer and exports nothing of it.  (libclipfsar_hip.so shares cfsar_fail
// etc. across its translation units by linkage instead: runtime.hip, which is not linked into the side libraries.)
#pragma once
#include <stdarg.h>

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

}  // namespace

#define SIDE_REQUIRE(cond, ...)               \
    do {                                      \
        if (!(cond)) return fail(__VA_ARGS__); \
    } while (0)
