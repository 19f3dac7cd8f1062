// rf_recover_common.hpp -- host helpers and the per-pixel arithmetic of librf_recover_hip.so (gfx950
// only).  The library shares no object with the other three: its error text and return codes are
// its own.
#pragma once
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>

#include "reflectance_filtering_recover.h"

namespace rfr {

// numerically the codes of reflectance_filtering.h
enum { kOk = 0, kBadArg = -1, kUnsupported = -2, kHip = -4 };

constexpr int kThreads = 256;   // four waves of 64

// Thread-local message behind rf_recover_last_error().
char *last_error_buf();
int fail(int code, const char *fmt, ...);

#define RFR_HIP_CHECK(expr)                                                                    \
    do {                                                                                       \
        hipError_t _e = (expr);                                                                \
        if (_e != hipSuccess)                                                                  \
            return ::rfr::fail(::rfr::kHip, "%s failed: %s (%s:%d)", #expr,                    \
                               hipGetErrorString(_e), __FILE__, __LINE__);                     \
    } while (0)

// The argument rules the three entries share; 0 or the refusal.
int check_sizes(const char *who, long long npixels, long long nlisted);
int check_norm(const char *who, int norm);

// What the recover layer keeps of one pixel.  Channel order R, G, B: the order of the reference's
// sums (x holds B, G, R).
struct Pixel {
    float ri_inv, m;
    float n[3];      // normalised image = d refl_c / d e
    float refl[3];
    float s, ds;     // shading and d s / d e
};

// np.maximum(v, EPS): the floor of the reference's _threshold.  Unlike fmaxf it hands a NaN on, so a diverged
// network shows in the losses and the gradient as it does in the reference.
__device__ __forceinline__ float floor_eps(float v)
{
    return v != v ? v : fmaxf(v, FLT_EPSILON);
}

__device__ __forceinline__ Pixel recover_pixel(float b, float g, float r, float e, int norm)
{
    Pixel p;
    const float ri = floor_eps(e);
    float v;
    if (norm == RF_RECOVER_NORM_MEAN)
        v = __fdiv_rn(__fadd_rn(__fadd_rn(r, g), b), 3.0f);
    else if (norm == RF_RECOVER_NORM_MAX)
        v = fmaxf(fmaxf(r, g), b);
    else if (norm == RF_RECOVER_NORM_Y)
        v = __fadd_rn(__fadd_rn(__fmul_rn(0.299f, r), __fmul_rn(0.587f, g)), __fmul_rn(0.114f, b));
    else
        // sqrtf, not __fsqrt_rn: the latter is the hardware's approximate square root in this toolchain, the
        // former is correctly rounded (hipcc's default -fhip-fp32-correctly-rounded-divide-sqrt)
        v = sqrtf(__fadd_rn(__fadd_rn(__fmul_rn(r, r), __fmul_rn(g, g)), __fmul_rn(b, b)));
    p.m = floor_eps(v);
    const float f = __fdiv_rn(1.0f, p.m);
    p.n[0] = __fmul_rn(f, r);
    p.n[1] = __fmul_rn(f, g);
    p.n[2] = __fmul_rn(f, b);
#pragma unroll
    for (int c = 0; c < 3; c++)
        p.refl[c] = __fmul_rn(ri, p.n[c]);
    p.ri_inv = __fdiv_rn(1.0f, ri);
    p.s = __fmul_rn(p.m, p.ri_inv);
    p.ds = __fmul_rn(-p.ri_inv, p.s);
    return p;
}

// ((c0 + c1) + c2) / 3: the boundary layer's intensity and the hinge layer's lightness
__device__ __forceinline__ float mean3(float c0, float c1, float c2)
{
    return __fdiv_rn(__fadd_rn(__fadd_rn(c0, c1), c2), 3.0f);
}

}  // namespace rfr
