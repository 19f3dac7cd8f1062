// rf_augment_common.hpp -- host helpers of librf_augment_hip.so (gfx950 only).  The library shares
// no object with librf_hip.so or librf_train_hip.so: its error text and return codes are its own.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>

#include "reflectance_filtering_augment.h"

namespace rfa {

// numerically the codes of reflectance_filtering.h
enum { kOk = 0, kBadArg = -1, kUnsupported = -2, kHip = -4 };

// Thread-local message behind rf_augment_last_error().
char *last_error_buf();
int fail(int code, const char *fmt, ...);

#define RFA_HIP_CHECK(expr)                                                                    \
    do {                                                                                       \
        hipError_t _e = (expr);                                                                \
        if (_e != hipSuccess)                                                                  \
            return ::rfa::fail(::rfa::kHip, "%s failed: %s (%s:%d)", #expr,                    \
                               hipGetErrorString(_e), __FILE__, __LINE__);                     \
    } while (0)

}  // namespace rfa
