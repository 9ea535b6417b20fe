// gol_error.h -- the library's error report and the check of a HIP call that ends in it (private).
// Apart from gol_internal.h, which holds the engine's state and with it the step launch table, so
// that the units that want only these two (the batch's host units) get nothing of the engine.
#pragma once
#include <hip/hip_runtime.h>

#include "golhip.h"

int gol_set_error(int code, const char *fmt, ...);

#define HIPCHK(expr)                                                                              \
    do {                                                                                          \
        hipError_t e_ = (expr);                                                                   \
        if (e_ != hipSuccess)                                                                     \
            return gol_set_error(e_ == hipErrorOutOfMemory ? GOL_ENOMEM : GOL_EHIP, "%s failed: %s (%s:%d)", #expr, \
                                 hipGetErrorString(e_), __FILE__, __LINE__);                      \
    } while (0)
