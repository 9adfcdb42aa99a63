// Host scaffolding of a side library's entry points (data.hip, det.hip, headfuse.hip, wslab.hip): the thread's last error text, the
// launch check and the argument check.  Everything here has internal linkage -- each library is one object and exports
// exactly what its header declares -- and nothing depends on include/madm_hip.h.  Every status enum has OK == 0; the
// library passes its own codes, and keeps a one-line  #define Mxx_REQUIRE(...) ENTRY_REQUIRE(Mxx_ERR_INVALID_ARG, __VA_ARGS__).
// libmadm_hip.so's madm_set_error / madm_check_launch are shared by its 21 objects and live in runtime.hip / common.hpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

static thread_local char g_err[512] = "";   // what the library's *_last_error() returns

static void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
}

static int check_launch(const char* what, int err_launch) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        set_error("%s: launch failed: %s", what, hipGetErrorString(e));
        return err_launch;
    }
    return 0;
}

#define ENTRY_REQUIRE(err_invalid_arg, cond, ...) \
    do {                                          \
        if (!(cond)) {                            \
            set_error(__VA_ARGS__);               \
            return err_invalid_arg;               \
        }                                         \
    } while (0)

static inline bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }
