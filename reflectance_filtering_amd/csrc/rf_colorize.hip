// rf_colorize.hip -- colourised reflectance / shading outputs of decompose_image, for gfx950.
//
// Replaces, for a batch that is already on the device, the host numpy chain of
// /root/reference/decompose_with_trained_CNN.py:121-128 and /root/reference/image_utils.py:60-92:
//
//   shading     = mean_c(image) / r                      (float64; image is the uint8 BGR input,
//   reflectance = image / max(shading, 1e-3)[..., None]   r the CNN's float32 intensity)
//   for out in (reflectance, shading):                   imwrite(..., sRGB=True)
//       if max(out) > 1: out = clip(out / percentile(out, 99.9, 'lower'), 0, 1)
//       out = rgb_to_srgb(out)                           (<= 0.0031308: *12.92,
//                                                          else (1.055*x)^(1/2.4) - 0.055)
//       bytes = (out * 255).astype(uint8)                (truncation)
//
// Everything is IEEE float64 and is reproduced operation by operation (one correctly rounded
// division / multiplication per numpy ufunc), with two exceptions that are made exact another way:
//  * the percentile is an order statistic (k-th smallest of the 3HW resp. HW values, k computed by
//    the host with numpy's own index rule): an 8-pass radix select on the bit patterns of the
//    non-negative doubles finds it without sorting and without storing the float64 images (they
//    are recomputed from the 7 input bytes per pixel in every pass);
//  * np.power is libm's pow, which the GPU cannot reproduce bit for bit.  But x -> byte is a
//    step function with at most 255 steps on the power branch, so the host computes the 255 step
//    positions once with numpy itself (image_utils.srgb_write_steps) and the kernel counts the
//    steps at or below x: exact for whatever libm the host has.
#include <type_traits>
#include <vector>

#include "reflectance_filtering_debug.h"
#include "rf_jbf_common.hpp"

namespace rf {
namespace {

struct SelState {
    unsigned long long prefix;  // high bits of the k-th smallest key found so far
    unsigned long long k;       // rank still to be located inside the current prefix bucket
    unsigned long long maxkey;  // largest key (for the `max > 1` test)
    unsigned int hist[256];
};

constexpr int kTargets = 2;  // 0: reflectance (3 values per pixel), 1: shading (1 per pixel)

__device__ inline unsigned long long key_of(double v) { return (unsigned long long)__double_as_longlong(v); }

// The float64 values numpy forms for one pixel.
__device__ inline void pixel_values(const uint8_t *px, float r, double (&refl)[3], double &shading)
{
    const double mean = __ddiv_rn((double)((int)px[0] + (int)px[1] + (int)px[2]), 3.0);
    shading = __ddiv_rn(mean, (double)r);
    const double den = shading > 1e-3 ? shading : (shading != shading ? shading : 1e-3);
#pragma unroll
    for (int c = 0; c < 3; c++)
        refl[c] = __ddiv_rn((double)px[c], den);
}

// The reflectance the kernels divide by: the float32 of the CNN as it is, or, for the entries that
// read an 8-bit map (rf_colorize_ragged_r8_srgb_u8), the float32 nearest to byte / 255 - the
// convention of rf_whdr_points_u8 - formed in registers from the one byte read per pixel.
__device__ __forceinline__ float reflectance_of(float r) { return r; }
__device__ __forceinline__ float reflectance_of(uint8_t r) { return __fdiv_rn((float)r, 255.0f); }

// what a call's first kernel leaves in one (image, target) state: everything the passes read
__device__ __forceinline__ void init_state(SelState &s, unsigned long long k)
{
    if (threadIdx.x == 0) {
        s.prefix = 0;
        s.k = k;
        s.maxkey = 0;
    }
    s.hist[threadIdx.x] = 0;
}

__global__ void colorize_init_kernel(SelState *st, int n, unsigned long long k_refl,
                                     unsigned long long k_shading)
{
    const int i = blockIdx.x;  // (image, target)
    init_state(st[i], (i % kTargets) == 0 ? k_refl : k_shading);
}

// One image of a ragged call (rf_colorize_ragged_srgb_u8): where its pixels start in the packed
// buffers, how many it has, its two percentile ranks and the first of its workgroups in the
// one-dimensional grid of the histogram and write kernels (ceil(npx / chunk_px) each, image order).
struct ColImage {
    unsigned long long first;  // pixels before the image
    unsigned long long npx;
    unsigned long long k_refl, k_shading;
    unsigned int wg0;
    unsigned int pad;
};
static_assert(sizeof(ColImage) == 40, "the workspace holds 40 bytes per image");

__global__ void colorize_ragged_init_kernel(SelState *st, const ColImage *__restrict__ images)
{
    const int i = blockIdx.x;  // (image, target)
    const ColImage &im = images[i / kTargets];
    init_state(st[i], (i % kTargets) == 0 ? im.k_refl : im.k_shading);
}

// The image a workgroup of the ragged kernels works on: the last one with wg0 <= blockIdx.x.
// Everything here depends on blockIdx.x alone, so the search runs on scalar loads.
__device__ __forceinline__ int ragged_image(const ColImage *__restrict__ images, int n)
{
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (images[mid].wg0 <= blockIdx.x)
            lo = mid;
        else
            hi = mid - 1;
    }
    return lo;
}

// pass p = 0..7 looks at key byte 7-p of the values whose higher bytes equal the prefix.
// One workgroup's share of one image: the pixels p0, p0 + step, ... below p1 of the image at b / rr,
// counted into the image's two states st[0..1].
template <typename R>
__device__ __forceinline__ void hist_pixels(const uint8_t *__restrict__ b, const R *__restrict__ rr,
                                            SelState *__restrict__ st, size_t p0, size_t p1,
                                            size_t step, int pass)
{
    __shared__ unsigned int hist[kTargets][256];
    __shared__ unsigned long long lmax[kTargets];
    hist[0][threadIdx.x] = 0;
    hist[1][threadIdx.x] = 0;
    if (threadIdx.x < kTargets)
        lmax[threadIdx.x] = 0;
    __syncthreads();
    const int shift = 56 - 8 * pass;
    const unsigned long long pre0 = st[0].prefix;
    const unsigned long long pre1 = st[1].prefix;
    unsigned long long m0 = 0, m1 = 0;
    for (size_t p = p0; p < p1; p += step) {
        double refl[3], sh;
        pixel_values(b + p * 3, reflectance_of(rr[p]), refl, sh);
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const unsigned long long k = key_of(refl[c]);
            if (pass == 0) {
                m0 = k > m0 ? k : m0;
                atomicAdd(&hist[0][k >> 56], 1u);
            } else if ((k >> (shift + 8)) == (pre0 >> (shift + 8))) {
                atomicAdd(&hist[0][(k >> shift) & 255u], 1u);
            }
        }
        const unsigned long long k = key_of(sh);
        if (pass == 0) {
            m1 = k > m1 ? k : m1;
            atomicAdd(&hist[1][k >> 56], 1u);
        } else if ((k >> (shift + 8)) == (pre1 >> (shift + 8))) {
            atomicAdd(&hist[1][(k >> shift) & 255u], 1u);
        }
    }
    if (pass == 0) {
        atomicMax(&lmax[0], m0);
        atomicMax(&lmax[1], m1);
    }
    __syncthreads();
#pragma unroll
    for (int t = 0; t < kTargets; t++) {
        const unsigned int c = hist[t][threadIdx.x];
        if (c)
            atomicAdd(&st[t].hist[threadIdx.x], c);
    }
    if (pass == 0 && threadIdx.x < kTargets)
        atomicMax(&st[threadIdx.x].maxkey, lmax[threadIdx.x]);
}

__global__ __launch_bounds__(256) void colorize_hist_kernel(const uint8_t *__restrict__ bgr,
                                                            const float *__restrict__ r,
                                                            SelState *__restrict__ st, size_t npx,
                                                            int pass)
{
    const int img = blockIdx.y;
    hist_pixels(bgr + (size_t)img * npx * 3, r + (size_t)img * npx, st + img * kTargets,
                (size_t)blockIdx.x * blockDim.x + threadIdx.x, npx, (size_t)gridDim.x * blockDim.x,
                pass);
}

// The same pass over images of different sizes: workgroup blockIdx.x takes one chunk of chunk_px
// consecutive pixels of one image.
__global__ __launch_bounds__(256) void colorize_ragged_hist_kernel(
    const uint8_t *__restrict__ bgr, const float *__restrict__ r, SelState *__restrict__ st,
    const ColImage *__restrict__ images, int n, unsigned int chunk_px, int pass)
{
    const int img = ragged_image(images, n);
    const ColImage &im = images[img];
    const size_t c0 = (size_t)(blockIdx.x - im.wg0) * chunk_px;
    const size_t c1 = c0 + chunk_px < im.npx ? c0 + chunk_px : (size_t)im.npx;
    hist_pixels(bgr + im.first * 3, r + im.first, st + img * kTargets, c0 + threadIdx.x, c1, 256,
                pass);
}

// ... and with an 8-bit reflectance map: the same pass, one byte read per pixel
__global__ __launch_bounds__(256) void colorize_ragged_hist_r8_kernel(
    const uint8_t *__restrict__ bgr, const uint8_t *__restrict__ r8, SelState *__restrict__ st,
    const ColImage *__restrict__ images, int n, unsigned int chunk_px, int pass)
{
    const int img = ragged_image(images, n);
    const ColImage &im = images[img];
    const size_t c0 = (size_t)(blockIdx.x - im.wg0) * chunk_px;
    const size_t c1 = c0 + chunk_px < im.npx ? c0 + chunk_px : (size_t)im.npx;
    hist_pixels(bgr + im.first * 3, r8 + im.first, st + img * kTargets, c0 + threadIdx.x, c1, 256,
                pass);
}

// one workgroup per (image, target): bucket that holds rank k, then clear the histogram
__global__ __launch_bounds__(256) void colorize_pick_kernel(SelState *st, int pass)
{
    SelState &s = st[blockIdx.x];
    __shared__ unsigned int h[256];
    h[threadIdx.x] = s.hist[threadIdx.x];
    __syncthreads();
    s.hist[threadIdx.x] = 0;
    if (threadIdx.x == 0) {
        unsigned long long k = s.k;
        int bin = 0;
        for (; bin < 255; bin++) {
            if (k < h[bin])
                break;
            k -= h[bin];
        }
        s.k = k;
        s.prefix |= (unsigned long long)bin << (56 - 8 * pass);
    }
}

// rgb_to_srgb + (x*255).astype(uint8) of a value in [0, steps[254]] (NaN -> 0 like the
// zero-initialised result array of the reference); above steps[254], where only a target holding
// a NaN goes unnormalised, 255 (numpy's cast overflows from byte 256 on)
__device__ inline uint8_t srgb_byte(double v, const double *__restrict__ steps)
{
    if (v <= 0.0031308)
        return (uint8_t)(int)__dmul_rn(__dmul_rn(v, 12.92), 255.0);
    if (!(v > 0.0031308))
        return 0;
    // number of steps k (1..255) with steps[k-1] <= v; the steps are non-decreasing
    int lo = 0, hi = 255;  // invariant: steps[lo-1] <= v < steps[hi]
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (steps[mid] <= v)
            lo = mid + 1;
        else
            hi = mid;
    }
    return (uint8_t)lo;
}

__device__ inline double normalise(double v, bool on, double pct)
{
    if (!on)
        return v;
    v = __ddiv_rn(v, pct);
    // np.clip(v, 0, 1) = minimum(maximum(v, 0), 1), NaN propagating
    if (v != v)
        return v;
    v = v < 0.0 ? 0.0 : v;
    return v > 1.0 ? 1.0 : v;
}

// One workgroup's share of one image, as hist_pixels: the bytes of the pixels p0, p0 + step, ...
// below p1 of the image at b / rr into refl_o / shading_o (the image's own outputs, or NULL).
template <typename R>
__device__ __forceinline__ void write_pixels(const uint8_t *__restrict__ b, const R *__restrict__ rr,
                                             const SelState *__restrict__ st,
                                             uint8_t *__restrict__ refl_o,
                                             uint8_t *__restrict__ shading_o, size_t p0, size_t p1,
                                             size_t step, const double *__restrict__ steps_g)
{
    __shared__ double steps[256];
    steps[threadIdx.x] = threadIdx.x < 255 ? steps_g[threadIdx.x] : __longlong_as_double(0x7ff0000000000000LL);
    __syncthreads();
    const SelState &s0 = st[0];
    const SelState &s1 = st[1];
    // np.max(img) > 1.  The values are non-negative, so the key of a NaN (exponent field all
    // ones, non-zero fraction) lies above that of +inf: np.max is NaN then, `NaN > 1` is false,
    // and the target is written without normalisation.
    const unsigned long long one = key_of(1.0), inf = key_of(__longlong_as_double(0x7ff0000000000000LL));
    const bool n0 = s0.maxkey > one && s0.maxkey <= inf;
    const bool n1 = s1.maxkey > one && s1.maxkey <= inf;
    const double pc0 = __longlong_as_double((long long)s0.prefix);
    const double pc1 = __longlong_as_double((long long)s1.prefix);
    for (size_t p = p0; p < p1; p += step) {
        double refl[3], sh;
        pixel_values(b + p * 3, reflectance_of(rr[p]), refl, sh);
        if (refl_o) {
            uint8_t *o = refl_o + p * 3;
#pragma unroll
            for (int c = 0; c < 3; c++)
                o[c] = srgb_byte(normalise(refl[c], n0, pc0), steps);
        }
        if (shading_o)
            shading_o[p] = srgb_byte(normalise(sh, n1, pc1), steps);
    }
}

__global__ __launch_bounds__(256) void colorize_write_kernel(
    const uint8_t *__restrict__ bgr, const float *__restrict__ r, const SelState *__restrict__ st,
    uint8_t *__restrict__ refl_out, uint8_t *__restrict__ shading_out, size_t npx,
    const double *__restrict__ steps_g)
{
    const size_t first = (size_t)blockIdx.y * npx;
    write_pixels(bgr + first * 3, r + first, st + blockIdx.y * kTargets,
                 refl_out ? refl_out + first * 3 : nullptr, shading_out ? shading_out + first : nullptr,
                 (size_t)blockIdx.x * blockDim.x + threadIdx.x, npx, (size_t)gridDim.x * blockDim.x,
                 steps_g);
}

__global__ __launch_bounds__(256) void colorize_ragged_write_kernel(
    const uint8_t *__restrict__ bgr, const float *__restrict__ r, const SelState *__restrict__ st,
    uint8_t *__restrict__ refl_out, uint8_t *__restrict__ shading_out,
    const ColImage *__restrict__ images, int n, unsigned int chunk_px,
    const double *__restrict__ steps_g)
{
    const int img = ragged_image(images, n);
    const ColImage &im = images[img];
    const size_t c0 = (size_t)(blockIdx.x - im.wg0) * chunk_px;
    const size_t c1 = c0 + chunk_px < im.npx ? c0 + chunk_px : (size_t)im.npx;
    write_pixels(bgr + im.first * 3, r + im.first, st + img * kTargets,
                 refl_out ? refl_out + im.first * 3 : nullptr,
                 shading_out ? shading_out + im.first : nullptr, c0 + threadIdx.x, c1, 256, steps_g);
}

__global__ __launch_bounds__(256) void colorize_ragged_write_r8_kernel(
    const uint8_t *__restrict__ bgr, const uint8_t *__restrict__ r8, const SelState *__restrict__ st,
    uint8_t *__restrict__ refl_out, uint8_t *__restrict__ shading_out,
    const ColImage *__restrict__ images, int n, unsigned int chunk_px,
    const double *__restrict__ steps_g)
{
    const int img = ragged_image(images, n);
    const ColImage &im = images[img];
    const size_t c0 = (size_t)(blockIdx.x - im.wg0) * chunk_px;
    const size_t c1 = c0 + chunk_px < im.npx ? c0 + chunk_px : (size_t)im.npx;
    write_pixels(bgr + im.first * 3, r8 + im.first, st + img * kTargets,
                 refl_out ? refl_out + im.first * 3 : nullptr,
                 shading_out ? shading_out + im.first : nullptr, c0 + threadIdx.x, c1, 256, steps_g);
}

// ---- the launch plan of the ragged entry (host) ----------------------------------------------

inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

// 256 threads per workgroup and a grid below 2^32 threads
constexpr unsigned long long kColMaxWorkgroups = (1ull << 24) - 1;

struct ColPlan {
    unsigned int chunk_px;            // pixels of one workgroup's chunk, one value per call
    unsigned long long workgroups;    // of the histogram and the write kernel
    std::vector<ColImage> images;
};

// The workspace: [image table, rounded up to 256 bytes][n x 2 SelState]
size_t ragged_table_bytes(int n) { return align256(sizeof(ColImage) * (size_t)n); }

// The argument rules of the sizes and ranks (k_refl / k_shading may both be NULL: a query without
// ranks) and the chunk rule: with T pixels in all, chunks of 2048 * ceil(T / (2048 * 65536)) pixels -
// 8 pixels per thread and at most 65536 + n workgroups, the two regimes of the uniform launch - or,
// where that makes fewer than 1024 workgroups, of 256 * ceil(T / (256 * 1024)) pixels.  The debug
// option "colorize_chunk_px" replaces the rule.  Touches no device.
int plan_ragged(const char *who, int n, const int *heights, const int *widths,
                const unsigned long long *k_refl, const unsigned long long *k_shading, ColPlan *plan)
{
    if (n < 0)
        return fail(RF_E_BADARG, "%s: bad size n=%d", who, n);
    if (n > 0 && (!heights || !widths))
        return fail(RF_E_BADARG, "%s: NULL pointer", who);
    plan->images.resize((size_t)n);
    unsigned long long total = 0;
    for (int i = 0; i < n; i++) {
        if (heights[i] <= 0 || widths[i] <= 0)
            return fail(RF_E_BADARG, "%s: bad size of image %d: h=%d w=%d", who, i, heights[i],
                        widths[i]);
        const unsigned long long npx = (unsigned long long)heights[i] * widths[i];
        if (3 * npx >= (1ull << 32))
            return fail(RF_E_UNSUPPORTED, "%s: image %d (%dx%d) holds 2^32 values or more: the "
                                          "histogram counters are 32 bits wide", who, i, widths[i],
                        heights[i]);
        if (k_refl && (k_refl[i] >= 3 * npx || k_shading[i] >= npx))
            return fail(RF_E_BADARG, "%s: percentile rank outside image %d", who, i);
        plan->images[i] = ColImage{total, npx, k_refl ? k_refl[i] : 0, k_refl ? k_shading[i] : 0, 0, 0};
        total += npx;
    }
    if (total > (1ull << 46))
        return fail(RF_E_UNSUPPORTED, "%s: the images hold too many pixels", who);
    auto count = [&](unsigned long long chunk) {
        unsigned long long wgs = 0;
        for (const ColImage &im : plan->images)
            wgs += (im.npx + chunk - 1) / chunk;
        return wgs;
    };
    auto ceil_div64 = [](unsigned long long a, unsigned long long b) { return (a + b - 1) / b; };
    unsigned long long chunk = (unsigned long long)debug_get(kDbgColorizeChunkPx);
    if (chunk != 0) {
        if (chunk % 256 != 0)
            return fail(RF_E_BADARG, "%s: debug option colorize_chunk_px = %llu is not a multiple of "
                                     "256", who, chunk);
    } else {
        chunk = 2048 * std::max<unsigned long long>(1, ceil_div64(total, 2048ull * 65536));
        if (count(chunk) < 1024)
            chunk = 256 * std::max<unsigned long long>(1, ceil_div64(total, 256ull * 1024));
    }
    plan->chunk_px = (unsigned int)chunk;
    plan->workgroups = 0;
    for (ColImage &im : plan->images) {
        if (plan->workgroups > kColMaxWorkgroups)
            break;
        im.wg0 = (unsigned int)plan->workgroups;
        plan->workgroups += (im.npx + chunk - 1) / chunk;
    }
    if (plan->workgroups > kColMaxWorkgroups || (unsigned long long)n * kTargets > kColMaxWorkgroups)
        return fail(RF_E_UNSUPPORTED, "%s: more workgroups than one grid takes (%llu)", who,
                    kColMaxWorkgroups);
    return RF_OK;
}

}  // namespace
}  // namespace rf

extern "C" size_t rf_colorize_workspace_bytes(int n)
{
    if (n <= 0)
        return 0;
    return (size_t)n * rf::kTargets * sizeof(rf::SelState);
}

extern "C" int rf_colorize_srgb_u8(const uint8_t *bgr, const float *r, uint8_t *refl_out,
                                   uint8_t *shading_out, int n, int h, int w,
                                   unsigned long long k_refl, unsigned long long k_shading,
                                   const double *srgb_steps, void *workspace,
                                   size_t workspace_bytes, void *stream_)
{
    using namespace rf;
    if (n == 0)
        return RF_OK;
    if (!bgr || !r || !srgb_steps || !workspace || (!refl_out && !shading_out))
        return fail(RF_E_BADARG, "rf_colorize_srgb_u8: NULL pointer");
    if (n < 0 || h <= 0 || w <= 0)
        return fail(RF_E_BADARG, "rf_colorize_srgb_u8: bad size n=%d h=%d w=%d", n, h, w);
    const size_t npx = (size_t)h * w;
    if (k_refl >= 3 * npx || k_shading >= npx)
        return fail(RF_E_BADARG, "rf_colorize_srgb_u8: percentile rank outside the image");
    if (workspace_bytes < rf_colorize_workspace_bytes(n))
        return fail(RF_E_WORKSPACE, "rf_colorize_srgb_u8: workspace %zu B < %zu B", workspace_bytes,
                    rf_colorize_workspace_bytes(n));
    if (n > 65535)
        return fail(RF_E_UNSUPPORTED, "rf_colorize_srgb_u8: n <= 65535 per call");
    hipStream_t stream = (hipStream_t)stream_;
    SelState *st = reinterpret_cast<SelState *>(workspace);
    hipLaunchKernelGGL(colorize_init_kernel, dim3(n * kTargets), dim3(256), 0, stream, st, n, k_refl,
                       k_shading);
    // enough workgroups to fill the chip, few enough that the per-block histogram flush is cheap
    int bx = (int)std::min<size_t>((npx + 256 * 8 - 1) / (256 * 8), 2048);
    if (bx * n < 1024)
        bx = (int)std::min<size_t>((npx + 255) / 256, (size_t)((1024 + n - 1) / n));
    if (bx < 1)
        bx = 1;
    for (int pass = 0; pass < 8; pass++) {
        hipLaunchKernelGGL(colorize_hist_kernel, dim3(bx, n), dim3(256), 0, stream, bgr, r, st, npx,
                           pass);
        hipLaunchKernelGGL(colorize_pick_kernel, dim3(n * kTargets), dim3(256), 0, stream, st, pass);
    }
    hipLaunchKernelGGL(colorize_write_kernel, dim3(bx, n), dim3(256), 0, stream, bgr, r, st, refl_out,
                       shading_out, npx, srgb_steps);
    RF_HIP_CHECK(hipGetLastError());
    return RF_OK;
}

extern "C" size_t rf_colorize_ragged_workspace_bytes(int n, const int *heights, const int *widths)
{
    using namespace rf;
    ColPlan plan;
    if (n <= 0 || plan_ragged("rf_colorize_ragged_workspace_bytes", n, heights, widths, nullptr,
                              nullptr, &plan) != RF_OK)
        return 0;
    return ragged_table_bytes(n) + (size_t)n * kTargets * sizeof(SelState);
}

extern "C" int rf_debug_colorize_ragged_plan(int n, const int *heights, const int *widths, int *out,
                                             int cap)
{
    using namespace rf;
    if (cap < 0 || (cap > 0 && !out))
        return fail(RF_E_BADARG, "rf_debug_colorize_ragged_plan: bad cap %d", cap);
    ColPlan plan;
    const int rc = plan_ragged("rf_debug_colorize_ragged_plan", n, heights, widths, nullptr, nullptr,
                               &plan);
    if (rc != RF_OK)
        return rc;
    if (cap > 0)
        out[0] = (int)plan.chunk_px;
    if (cap > 1)
        out[1] = (int)plan.workgroups;
    for (int i = 0; i < n && i + 2 < cap; i++)
        out[i + 2] = (int)plan.images[i].wg0;
    return n;
}

namespace rf {
namespace {

// The ragged entries: `r` is the float32 map of rf_colorize_ragged_srgb_u8 or the 8-bit map of
// rf_colorize_ragged_r8_srgb_u8; everything but the two kernels that read it is shared.
template <typename R>
int colorize_ragged(const char *who, const uint8_t *bgr, const R *r, uint8_t *refl_out,
                    uint8_t *shading_out, int n, const int *heights, const int *widths,
                    const unsigned long long *k_refl, const unsigned long long *k_shading,
                    const double *srgb_steps, void *workspace, size_t workspace_bytes, void *stream_)
{
    if (n == 0)
        return RF_OK;
    if (!bgr || !r || !srgb_steps || !workspace || !heights || !widths || !k_refl || !k_shading ||
        (!refl_out && !shading_out))
        return fail(RF_E_BADARG, "%s: NULL pointer", who);
    ColPlan plan;
    const int rc = plan_ragged(who, n, heights, widths, k_refl, k_shading, &plan);
    if (rc != RF_OK)
        return rc;
    const size_t off_states = ragged_table_bytes(n);
    const size_t need = off_states + (size_t)n * kTargets * sizeof(SelState);
    if (workspace_bytes < need)
        return fail(RF_E_WORKSPACE, "%s: workspace %zu B < %zu B", who, workspace_bytes, need);
    if ((uintptr_t)workspace % 16 != 0)
        return fail(RF_E_BADARG, "%s: the workspace must be 16-byte aligned", who);
    hipStream_t stream = (hipStream_t)stream_;
    if (stream_is_capturing(stream))
        return fail(RF_E_UNSUPPORTED, "%s: synchronises its stream and cannot be captured into a "
                                      "graph", who);
    // the host table must outlive the copy: the copy is waited for before the launches (this is
    // the call's one synchronisation of `stream`)
    RF_HIP_CHECK(hipMemcpyAsync(workspace, plan.images.data(), sizeof(ColImage) * (size_t)n,
                                hipMemcpyHostToDevice, stream));
    RF_HIP_CHECK(hipStreamSynchronize(stream));
    const ColImage *images = reinterpret_cast<const ColImage *>(workspace);
    SelState *st = reinterpret_cast<SelState *>(static_cast<char *>(workspace) + off_states);
    const dim3 grid((unsigned int)plan.workgroups);
    constexpr bool kBytes = std::is_same<R, uint8_t>::value;
    hipLaunchKernelGGL(colorize_ragged_init_kernel, dim3(n * kTargets), dim3(256), 0, stream, st,
                       images);
    for (int pass = 0; pass < 8; pass++) {
        if constexpr (kBytes)
            hipLaunchKernelGGL(colorize_ragged_hist_r8_kernel, grid, dim3(256), 0, stream, bgr, r, st,
                               images, n, plan.chunk_px, pass);
        else
            hipLaunchKernelGGL(colorize_ragged_hist_kernel, grid, dim3(256), 0, stream, bgr, r, st,
                               images, n, plan.chunk_px, pass);
        hipLaunchKernelGGL(colorize_pick_kernel, dim3(n * kTargets), dim3(256), 0, stream, st, pass);
    }
    if constexpr (kBytes)
        hipLaunchKernelGGL(colorize_ragged_write_r8_kernel, grid, dim3(256), 0, stream, bgr, r, st,
                           refl_out, shading_out, images, n, plan.chunk_px, srgb_steps);
    else
        hipLaunchKernelGGL(colorize_ragged_write_kernel, grid, dim3(256), 0, stream, bgr, r, st,
                           refl_out, shading_out, images, n, plan.chunk_px, srgb_steps);
    RF_HIP_CHECK(hipGetLastError());
    return RF_OK;
}

}  // namespace
}  // namespace rf

extern "C" int rf_colorize_ragged_srgb_u8(const uint8_t *bgr, const float *r, uint8_t *refl_out,
                                          uint8_t *shading_out, int n, const int *heights,
                                          const int *widths, const unsigned long long *k_refl,
                                          const unsigned long long *k_shading,
                                          const double *srgb_steps, void *workspace,
                                          size_t workspace_bytes, void *stream)
{
    return rf::colorize_ragged("rf_colorize_ragged_srgb_u8", bgr, r, refl_out, shading_out, n, heights,
                               widths, k_refl, k_shading, srgb_steps, workspace, workspace_bytes,
                               stream);
}

extern "C" int rf_colorize_ragged_r8_srgb_u8(const uint8_t *bgr, const uint8_t *r8, uint8_t *refl_out,
                                             uint8_t *shading_out, int n, const int *heights,
                                             const int *widths, const unsigned long long *k_refl,
                                             const unsigned long long *k_shading,
                                             const double *srgb_steps, void *workspace,
                                             size_t workspace_bytes, void *stream)
{
    return rf::colorize_ragged("rf_colorize_ragged_r8_srgb_u8", bgr, r8, refl_out, shading_out, n,
                               heights, widths, k_refl, k_shading, srgb_steps, workspace,
                               workspace_bytes, stream);
}
