// rf_whdr.hip -- WHDR of a batch of reflectance predictions against IIW judgements (gfx950).
//
// Replaces the per-comparison Python loop of /root/reference/training/layers/whdr_layer.py:253-287
// (with _lightness, :180-196) for device-resident predictions: one wave per image; lanes decide
// 64 comparisons at a time (two point gathers, float32 lightness = max(eps, mean over channels),
// float32 ratios against float32(1 + delta)), lane 0 then adds the weights in comparison order in
// float64, which is the order and precision of the reference's scalar accumulation.
#include <cfloat>

#include "rf_common.hpp"

namespace rf {
namespace {

// Python's max(eps, m): m only if m > eps
__device__ inline float lightness_floor(float m) { return m > FLT_EPSILON ? m : FLT_EPSILON; }

// np.mean of a float32 3-vector: ((r0 + r1) + r2) / 3 in float32
__device__ inline float mean3(float a, float b, float c)
{
    return __fdiv_rn(__fadd_rn(__fadd_rn(a, b), c), 3.0f);
}

__device__ inline float lightness(const float *__restrict__ img, int c, size_t plane, size_t pix)
{
    const float m = c == 3 ? mean3(img[pix], img[plane + pix], img[2 * plane + pix]) : img[pix];
    return lightness_floor(m);
}

// The same for a uint8 pixel (c interleaved bytes): each byte is (float)byte / 255.0f, correctly
// rounded - the value numpy's float32 `bytes / np.float32(255)` gives.
__device__ inline float lightness_u8(const uint8_t *__restrict__ px, int c)
{
    const float b0 = __fdiv_rn((float)px[0], 255.0f);
    if (c != 3)
        return lightness_floor(b0);
    return lightness_floor(
        mean3(b0, __fdiv_rn((float)px[1], 255.0f), __fdiv_rn((float)px[2], 255.0f)));
}

// The image's verdict on a pair: 1 = point 1 darker, 2 = point 2 darker, 0 = about equal.
__device__ inline int whdr_verdict(float l1, float l2, float thresh)
{
    if (__fdiv_rn(l2, l1) > thresh)
        return 1;
    if (__fdiv_rn(l1, l2) > thresh)
        return 2;
    return 0;
}

// WHDR of comparisons [k0, k1) on one 64-lane workgroup: lanes decide 64 comparisons at a time
// (error(k) = the weight of comparison k if the image disagrees with it, else 0), lane 0 adds the
// weights in comparison order in float64.  Returns the rate on lane 0.
template <class ErrorOf>
__device__ inline double whdr_wave(int k0, int k1, const double *__restrict__ wts, ErrorOf error)
{
    __shared__ double err_w[64];
    const int lane = threadIdx.x;
    double error_sum = 0.0, weight_sum = 0.0;
    for (int base = k0; base < k1; base += 64) {
        const int k = base + lane;
        err_w[lane] = k < k1 ? error(k) : 0.0;
        __syncthreads();
        if (lane == 0) {
            const int cnt = min(64, k1 - base);
            for (int j = 0; j < cnt; j++) {
                // `error_sum += weight` only happens on a mismatch; adding +0.0 otherwise leaves
                // the (non-negative) running sum unchanged
                error_sum += err_w[j];
                weight_sum += wts[base + j];
            }
        }
        __syncthreads();
    }
    return weight_sum != 0.0 ? error_sum / weight_sum : 0.0;
}

__global__ __launch_bounds__(64) void whdr_kernel(const float *__restrict__ refl, int c, int h,
                                                  int w, const int *__restrict__ pts,
                                                  const double *__restrict__ wts,
                                                  const int *__restrict__ offsets, float thresh,
                                                  double *__restrict__ out)
{
    const int img = blockIdx.x;
    const size_t plane = (size_t)h * w;
    const float *R = refl + (size_t)img * c * plane;
    const double r = whdr_wave(offsets[img], offsets[img + 1], wts, [&](int k) {
        const int *p = pts + (size_t)k * 5;
        const float l1 = lightness(R, c, plane, (size_t)p[1] * w + p[0]);
        const float l2 = lightness(R, c, plane, (size_t)p[3] * w + p[2]);
        return p[4] != whdr_verdict(l1, l2, thresh) ? wts[k] : 0.0;
    });
    if (threadIdx.x == 0)
        out[img] = r;
}

// One workgroup per (set, image): comparisons index the image's points, the points of image i of
// set s being the pixels s * set_stride + point_offsets[i] + index of `samples`.
__global__ __launch_bounds__(64) void whdr_points_kernel(
    const uint8_t *__restrict__ samples, long long set_stride, int c, int n,
    const int *__restrict__ point_offsets, const int *__restrict__ comps,
    const double *__restrict__ wts, const int *__restrict__ comp_offsets, float thresh,
    double *__restrict__ out)
{
    const int img = blockIdx.x % n;
    const int set = blockIdx.x / n;
    const uint8_t *S = samples + (size_t)set * set_stride * c;
    const long long first = point_offsets[img];
    const double r = whdr_wave(comp_offsets[img], comp_offsets[img + 1], wts, [&](int k) {
        const int *p = comps + (size_t)k * 3;
        // indices are validated by the caller; clamping keeps every read inside the set anyway
        const long long q1 = min(max(first + p[0], 0ll), set_stride - 1);
        const long long q2 = min(max(first + p[1], 0ll), set_stride - 1);
        const float l1 = lightness_u8(S + (size_t)q1 * c, c);
        const float l2 = lightness_u8(S + (size_t)q2 * c, c);
        return p[2] != whdr_verdict(l1, l2, thresh) ? wts[k] : 0.0;
    });
    if (threadIdx.x == 0)
        out[blockIdx.x] = r;
}

}  // namespace
}  // namespace rf

extern "C" int rf_whdr_f32(const float *refl, int n, int c, int h, int w, const int *points,
                           const double *weights, const int *offsets, double delta, double *out,
                           void *stream_)
{
    using namespace rf;
    if (n == 0)
        return RF_OK;
    if (!refl || !points || !weights || !offsets || !out)
        return fail(RF_E_BADARG, "rf_whdr_f32: NULL pointer");
    if (n < 0 || h <= 0 || w <= 0)
        return fail(RF_E_BADARG, "rf_whdr_f32: bad size n=%d h=%d w=%d", n, h, w);
    if (c != 1 && c != 3)
        return fail(RF_E_UNSUPPORTED, "rf_whdr_f32: 1 or 3 channels (got %d)", c);
    if (!(delta >= 0))
        return fail(RF_E_BADARG, "rf_whdr_f32: delta must be >= 0");
    if (!launch_fits((unsigned long long)n, 64))
        return fail(RF_E_UNSUPPORTED, "rf_whdr_f32: n too large for one launch");
    const float thresh = (float)(1.0 + delta);
    hipLaunchKernelGGL(whdr_kernel, dim3(n), dim3(64), 0, (hipStream_t)stream_, refl, c, h, w,
                       points, weights, offsets, thresh, out);
    RF_HIP_CHECK(hipGetLastError());
    return RF_OK;
}

extern "C" int rf_whdr_points_u8(const uint8_t *samples, int n_sets, long long set_stride, int c,
                                 int n, const int *point_offsets, const int *comps,
                                 const double *weights, const int *comp_offsets, double delta,
                                 double *out, void *stream_)
{
    using namespace rf;
    if (n == 0)
        return RF_OK;
    if (!samples || !point_offsets || !comps || !weights || !comp_offsets || !out)
        return fail(RF_E_BADARG, "rf_whdr_points_u8: NULL pointer");
    if (n < 0 || n_sets <= 0 || set_stride <= 0)
        return fail(RF_E_BADARG, "rf_whdr_points_u8: bad size n=%d n_sets=%d set_stride=%lld", n,
                    n_sets, set_stride);
    if (!launch_fits((unsigned long long)n * n_sets, 64))
        return fail(RF_E_UNSUPPORTED, "rf_whdr_points_u8: n * n_sets too large for one launch");
    if (c != 1 && c != 3)
        return fail(RF_E_UNSUPPORTED, "rf_whdr_points_u8: 1 or 3 channels (got %d)", c);
    if (!(delta >= 0))
        return fail(RF_E_BADARG, "rf_whdr_points_u8: delta must be >= 0");
    const float thresh = (float)(1.0 + delta);
    hipLaunchKernelGGL(whdr_points_kernel, dim3(n * n_sets), dim3(64), 0, (hipStream_t)stream_,
                       samples, set_stride, c, n, point_offsets, comps, weights, comp_offsets,
                       thresh, out);
    RF_HIP_CHECK(hipGetLastError());
    return RF_OK;
}
