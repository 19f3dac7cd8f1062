// rf_gf_f32.hip -- the CV_32F guided filter (rf_gf_f32) for gfx950: its own kernels around the
// row-sum / column-sum pair of rf_gf_twokernel.hpp and the per-pixel algebra of rf_gf_algebra.hpp.
// rf_gf_u8 runs it on float copies of 8-bit images at radii beyond the 8-bit kernels' range
// (rf_gf.hip).
#include <algorithm>

#include "rf_gf_algebra.hpp"
#include "rf_gf_common.hpp"
#include "rf_gf_twokernel.hpp"

namespace rf {
namespace {

// ------------------------------------------------------------------------------------------
// CV_32F variant.  Same operations as the uint8 path, but the stage-1 window
// sums are no longer exact integers, so every box filter is the order-faithful pair
// RowSum<float,double> / ColumnSum<double,float>: products -> row sums -> column sums -> means
// -> per-pixel algebra -> row sums -> column sums + apply.
// ------------------------------------------------------------------------------------------
// P: [img][NQ][h][w], quantity order of Quant<SCN>
template <int SCN>
__global__ __launch_bounds__(256) void gff_products_kernel(const float *__restrict__ guide,
                                                           const float *__restrict__ src,
                                                           float *__restrict__ P, size_t npx)
{
    constexpr int NQ = Quant<SCN>::NQ;
    const size_t pix = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (pix >= npx)
        return;
    const float *g = guide + ((size_t)blockIdx.y * npx + pix) * 3;
    const float *p = src + ((size_t)blockIdx.y * npx + pix) * SCN;
    float *out = P + (size_t)blockIdx.y * NQ * npx + pix;
    const float g0 = g[0], g1 = g[1], g2 = g[2];
    out[0 * npx] = g0;
    out[1 * npx] = g1;
    out[2 * npx] = g2;
    out[3 * npx] = __fmul_rn(g0, g0);
    out[4 * npx] = __fmul_rn(g0, g1);
    out[5 * npx] = __fmul_rn(g0, g2);
    out[6 * npx] = __fmul_rn(g1, g1);
    out[7 * npx] = __fmul_rn(g1, g2);
    out[8 * npx] = __fmul_rn(g2, g2);
#pragma unroll
    for (int s = 0; s < SCN; s++) {
        const float ps = p[s];
        out[(size_t)(9 + s) * npx] = ps;
        out[(size_t)(9 + SCN + 3 * s + 0) * npx] = __fmul_rn(ps, g0);
        out[(size_t)(9 + SCN + 3 * s + 1) * npx] = __fmul_rn(ps, g1);
        out[(size_t)(9 + SCN + 3 * s + 2) * npx] = __fmul_rn(ps, g2);
    }
}

// ColumnSum<double,float>: rowsums [img][np][h][w] -> means [img][np][h][w]; one lane per column
// of one plane.  grid (ceil(w/64), np, images)
__global__ __launch_bounds__(64) void gff_colsum_mean_kernel(const double *__restrict__ rowsums,
                                                             float *__restrict__ means, int h,
                                                             int w, int radius, int np)
{
    const int x = blockIdx.x * 64 + threadIdx.x;
    if (x >= w)
        return;
    const size_t npx = (size_t)h * w;
    const size_t plane = (size_t)blockIdx.z * np + blockIdx.y;
    const double *R = rowsums + plane * npx + x;
    float *M = means + plane * npx + x;
    const int ks = 2 * radius + 1;
    const double scale = 1.0 / (double)(ks * ks);
    double SUM = 0.0;
    for (int yy = -radius; yy < radius; yy++)
        SUM += R[(size_t)border_interpolate(yy, h, RF_BORDER_REFLECT) * w];
    for (int y = 0; y < h; y++) {
        const double s0 = SUM + R[(size_t)border_interpolate(y + radius, h, RF_BORDER_REFLECT) * w];
        M[(size_t)y * w] = (float)(s0 * scale);
        SUM = s0 - R[(size_t)border_interpolate(y - radius, h, RF_BORDER_REFLECT) * w];
    }
}

// means [img][NQ][h][w] -> alpha/beta in place in the first 4*SCN planes of each image
template <int SCN>
__global__ __launch_bounds__(256) void gff_algebra_kernel(float *__restrict__ P, size_t npx,
                                                          float eps_f, int eps_small)
{
    constexpr int NQ = Quant<SCN>::NQ;
    const size_t pix = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (pix >= npx)
        return;
    float *base = P + (size_t)blockIdx.y * NQ * npx + pix;
    float m[NQ], ab[4 * SCN];
#pragma unroll
    for (int q = 0; q < NQ; q++)
        m[q] = base[(size_t)q * npx];
    gf_pixel_algebra<SCN>(m, eps_f, eps_small, ab);
#pragma unroll
    for (int e = 0; e < 4 * SCN; e++)
        base[(size_t)e * npx] = ab[e];
}

template <int SCN>
int gf_f32_chunk(const float *guide, const float *src, float *dst, int m, int h, int w, int radius,
                 float eps_f, int eps_small, int iterations, float *P, double *rows,
                 hipStream_t stream)
{
    constexpr int NQ = Quant<SCN>::NQ;
    const size_t npx = (size_t)h * w;
    const int row_blocks = ceil_div(h, kBRows);
    const unsigned pb = (unsigned)((npx + 255) / 256);
    for (int it = 0; it < iterations; it++) {
        const float *s0 = it == 0 ? src : dst;
        hipLaunchKernelGGL(gff_products_kernel<SCN>, dim3(pb, m), dim3(256), 0, stream, guide, s0, P,
                           npx);
        hipLaunchKernelGGL(gf_rowsum_kernel<1>, dim3((unsigned)(m * NQ * row_blocks)), dim3(64), 0,
                           stream, P, rows, h, w, radius, row_blocks, NQ, (const int *)nullptr, NQ);
        hipLaunchKernelGGL(gff_colsum_mean_kernel, dim3(ceil_div(w, 64), NQ, m), dim3(64), 0, stream,
                           rows, P, h, w, radius, NQ);
        hipLaunchKernelGGL(gff_algebra_kernel<SCN>, dim3(pb, m), dim3(256), 0, stream, P, npx, eps_f,
                           eps_small);
        hipLaunchKernelGGL(gf_rowsum_kernel<1>, dim3((unsigned)(m * 4 * SCN * row_blocks)), dim3(64), 0,
                           stream, P, rows, h, w, radius, row_blocks, 4 * SCN,
                           (const int *)nullptr, NQ);
        hipLaunchKernelGGL((gf_colsum_apply_kernel<SCN, SCN, float>), dim3(ceil_div(w, 64), 1, m),
                           dim3(64, 4 * SCN), 0, stream, rows, guide, dst, h, w, radius,
                           (const int *)nullptr, 3);
    }
    return RF_OK;
}

}  // namespace
}  // namespace rf

extern "C" size_t rf_gf_f32_workspace_bytes(int n, int h, int w, int guide_cn, int src_cn,
                                            int radius)
{
    (void)guide_cn;
    (void)radius;
    if (n <= 0 || h <= 0 || w <= 0 || (src_cn != 1 && src_cn != 3))
        return 0;
    const size_t per_img = (size_t)h * w * (9 + 4 * src_cn) * (sizeof(float) + sizeof(double));
    size_t imgs = (size_t)n;
    const size_t cap = (size_t)16 << 30;
    if (imgs * per_img > cap)
        imgs = cap / per_img;
    if (imgs < 1)
        imgs = 1;
    return imgs * per_img;
}

extern "C" int rf_gf_f32(const float *guide, const float *src, float *dst, int n, int h, int w,
                         int guide_cn, int src_cn, int radius, double eps, int iterations,
                         void *workspace, size_t workspace_bytes, void *stream_)
{
    using namespace rf;
    const char *who = "rf_gf_f32";
    if (n == 0)
        return RF_OK;
    if (!guide || !src || !dst || !workspace)
        return fail(RF_E_BADARG, "%s: NULL pointer", who);
    if (n < 0 || h <= 0 || w <= 0 || iterations < 1)
        return fail(RF_E_BADARG, "%s: bad size n=%d h=%d w=%d iterations=%d", who, n, h, w, iterations);
    if (int bad = gf_check_guide(who, guide_cn, false))
        return bad;
    if (int bad = gf_check_src_cn(who, src_cn))
        return bad;
    if (int bad = gf_check_radius(who, radius))
        return bad;
    if (int bad = gf_check_overlap(who, guide, src, dst, (size_t)n * h * w, 3, src_cn, sizeof(float)))
        return bad;
    const int nq = 9 + 4 * src_cn;
    const size_t npx = (size_t)h * w;
    const size_t per_img = npx * nq * (sizeof(float) + sizeof(double));
    if (workspace_bytes < per_img)
        return fail(RF_E_WORKSPACE, "rf_gf_f32: workspace %zu B < %zu B needed for one image",
                    workspace_bytes, per_img);
    hipStream_t stream = (hipStream_t)stream_;
    int chunk = (int)std::min<size_t>((size_t)n, workspace_bytes / per_img);
    // gf_f32_chunk puts the image index in gridDim.y / .z and folds the chunk into gridDim.x
    chunk = gf_launch_chunk(std::min(chunk, kMaxGridYZ), h, w, src_cn, true);
    if (chunk == 0)
        return fail(RF_E_UNSUPPORTED, "rf_gf_f32: an image of %d x %d is too large for one launch", w, h);
    for (int i0 = 0; i0 < n; i0 += chunk) {
        const int m = std::min(chunk, n - i0);
        double *rows = reinterpret_cast<double *>(workspace);
        float *P = reinterpret_cast<float *>(rows + (size_t)m * nq * npx);
        const float *g0 = guide + (size_t)i0 * npx * 3;
        const float *s0 = src + (size_t)i0 * npx * src_cn;
        float *d0 = dst + (size_t)i0 * npx * src_cn;
        const int rc = src_cn == 3 ? gf_f32_chunk<3>(g0, s0, d0, m, h, w, radius, (float)eps,
                                                     eps < 1e-2, iterations, P, rows, stream)
                                   : gf_f32_chunk<1>(g0, s0, d0, m, h, w, radius, (float)eps,
                                                     eps < 1e-2, iterations, P, rows, stream);
        if (rc != RF_OK)
            return rc;
    }
    RF_HIP_CHECK(hipGetLastError());
    return RF_OK;
}
