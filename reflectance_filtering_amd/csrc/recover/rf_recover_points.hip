// rf_recover_points.hip -- the recover layer at listed pixels (lightness, reflectance, shading) and
// the hinge loss's gradient scattered back into grad_e at those pixels.
//
// Both kernels are gathers of a few thousand judgement points out of a dense buffer: one thread per
// listed pixel reads its three dwords of x directly (a gathered pixel shares its cache line with no
// other listed one, so there is nothing to stage).
#include "rf_recover_common.hpp"

namespace rfr {
namespace {

__global__ __launch_bounds__(kThreads) void recover_forward_kernel(
    const float *__restrict__ x, const float *__restrict__ e, const long long *__restrict__ pixel,
    int nlisted, int norm, float *__restrict__ lightness, float *__restrict__ reflectance,
    float *__restrict__ shading)
{
    const size_t k = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (k >= (size_t)nlisted)
        return;
    const size_t q = pixel ? (size_t)pixel[k] : k;
    const Pixel p = recover_pixel(x[3 * q], x[3 * q + 1], x[3 * q + 2], e[q], norm);
    if (lightness)
        lightness[k] = floor_eps(mean3(p.refl[0], p.refl[1], p.refl[2]));
    if (reflectance) {
        reflectance[3 * k] = p.refl[2];
        reflectance[3 * k + 1] = p.refl[1];
        reflectance[3 * k + 2] = p.refl[0];
    }
    if (shading)
        shading[k] = p.s;
}

__global__ __launch_bounds__(kThreads) void hinge_scatter_kernel(
    const float *__restrict__ x, const float *__restrict__ e, const float *__restrict__ grad_l,
    const long long *__restrict__ pixel, int nlisted, int norm, float scale, float *grad_e)
{
    const size_t k = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (k >= (size_t)nlisted)
        return;
    const size_t q = (size_t)pixel[k];
    const Pixel p = recover_pixel(x[3 * q], x[3 * q + 1], x[3 * q + 2], e[q], norm);
    const float g = __fdiv_rn(__fmul_rn(scale, grad_l[k]), 3.0f);
    const float add = __fadd_rn(__fadd_rn(__fmul_rn(g, p.n[0]), __fmul_rn(g, p.n[1])),
                                __fmul_rn(g, p.n[2]));
    grad_e[q] = __fadd_rn(grad_e[q], add);
}

}  // namespace
}  // namespace rfr

extern "C" int rf_recover_forward_f32(const float *x, const float *e, long long npixels,
                                      const long long *pixel, long long nlisted, int norm,
                                      float *lightness, float *reflectance, float *shading,
                                      void *stream_)
{
    using namespace rfr;
    const char *who = "rf_recover_forward_f32";
    if (int bad = check_sizes(who, npixels, nlisted))
        return bad;
    if (npixels == 0 || nlisted == 0)  // nothing listed: valid whatever the pointers are
        return kOk;
    if (!x || !e)
        return fail(kBadArg, "%s: NULL pointer", who);
    if (int bad = check_norm(who, norm))
        return bad;
    if (!pixel && nlisted > npixels)
        return fail(kBadArg, "%s: bad size K=%lld > P=%lld without a pixel list", who, nlisted, npixels);
    const unsigned blocks = (unsigned)((nlisted + kThreads - 1) / kThreads);
    hipLaunchKernelGGL(recover_forward_kernel, dim3(blocks), dim3(kThreads), 0, (hipStream_t)stream_,
                       x, e, pixel, (int)nlisted, norm, lightness, reflectance, shading);
    RFR_HIP_CHECK(hipGetLastError());
    return kOk;
}

extern "C" int rf_recover_hinge_scatter_f32(const float *x, const float *e, const float *grad_l,
                                            const long long *pixel, long long nlisted,
                                            long long npixels, int norm, float scale, float *grad_e,
                                            void *stream_)
{
    using namespace rfr;
    const char *who = "rf_recover_hinge_scatter_f32";
    if (int bad = check_sizes(who, npixels, nlisted))
        return bad;
    if (npixels == 0 || nlisted == 0)
        return kOk;
    if (!x || !e || !grad_l || !pixel || !grad_e)
        return fail(kBadArg, "%s: NULL pointer", who);
    if (int bad = check_norm(who, norm))
        return bad;
    if (!std::isfinite(scale))
        return fail(kBadArg, "%s: the scale must be finite", who);
    const unsigned blocks = (unsigned)((nlisted + kThreads - 1) / kThreads);
    hipLaunchKernelGGL(hinge_scatter_kernel, dim3(blocks), dim3(kThreads), 0, (hipStream_t)stream_,
                       x, e, grad_l, pixel, (int)nlisted, norm, scale, grad_e);
    RFR_HIP_CHECK(hipGetLastError());
    return kOk;
}
