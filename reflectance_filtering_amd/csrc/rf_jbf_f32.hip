// rf_jbf_f32.hip -- the CV_32F joint bilateral filter: jointBilateralFilter_32f.
// The colour weight is linearly interpolated in a per-image table of 4096 bins per joint channel
// over the joint's value range.  jbf_f32_quad_kernel (register-tiled, tables in LDS) whenever its
// tables fit; jbf_f32_kernel (one thread per output pixel) otherwise and as the cross-check.  Tap
// offsets and spatial weights are the tables of the 8-bit path (rf_jbf_tables.hpp); no kernel or
// launcher is shared with it.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <type_traits>
#include <vector>

#include "rf_jbf_common.hpp"
#include "rf_jbf_tables.hpp"

namespace rf {
namespace {

constexpr int kF32BinsPerChannel = 1 << 12;

// order-preserving map of a float's bits to uint32
__device__ inline uint32_t ordered_bits(float v)
{
    const uint32_t b = __float_as_uint(v);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
inline float from_ordered_bits(uint32_t k)
{
    const uint32_t b = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
    float v;
    __builtin_memcpy(&v, &b, 4);
    return v;
}

// minmax[2*img] = min, [2*img+1] = max (ordered bits); initialised to 0xffffffff / 0
__global__ __launch_bounds__(256) void jbf_f32_minmax_kernel(const float *__restrict__ joint,
                                                             uint32_t *__restrict__ minmax,
                                                             size_t count)
{
    const float *p = joint + (size_t)blockIdx.y * count;
    uint32_t lo = 0xffffffffu, hi = 0u;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < count;
         i += (size_t)gridDim.x * blockDim.x) {
        const uint32_t k = ordered_bits(p[i]);
        lo = min(lo, k);
        hi = max(hi, k);
    }
    atomicMin(&minmax[2 * blockIdx.y], lo);
    atomicMax(&minmax[2 * blockIdx.y + 1], hi);
}

template <int JCN, int SCN>
__global__ __launch_bounds__(256) void jbf_f32_kernel(
    const float *__restrict__ joint, const float *__restrict__ src, float *__restrict__ dst, int h,
    int w, int border, const float *__restrict__ luts, int lut_stride,
    const float *__restrict__ scales, const int *__restrict__ di, const int *__restrict__ dj,
    const float *__restrict__ sw, int maxk)
{
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= w || y >= h)
        return;
    const size_t img = (size_t)blockIdx.z * h * w;
    const float *lut = luts + (size_t)blockIdx.z * lut_stride;
    const float scale_index = scales[blockIdx.z];
    float j0[JCN];
#pragma unroll
    for (int c = 0; c < JCN; c++)
        j0[c] = joint[(img + (size_t)y * w + x) * JCN + c];
    float sum[SCN];
#pragma unroll
    for (int c = 0; c < SCN; c++)
        sum[c] = 0.f;
    float wsum = 0.f;
    for (int k = 0; k < maxk; k++) {
        const int yy = border_interpolate(y + di[k], h, border);
        const int xx = border_interpolate(x + dj[k], w, border);
        float jt[JCN], st[SCN];
#pragma unroll
        for (int c = 0; c < JCN; c++)
            jt[c] = 0.f;
#pragma unroll
        for (int c = 0; c < SCN; c++)
            st[c] = 0.f;
        if (yy >= 0 && xx >= 0) {
            const size_t q = img + (size_t)yy * w + xx;
#pragma unroll
            for (int c = 0; c < JCN; c++)
                jt[c] = joint[q * JCN + c];
#pragma unroll
            for (int c = 0; c < SCN; c++)
                st[c] = src[q * SCN + c];
        }
        float alpha = 0.f;
#pragma unroll
        for (int c = 0; c < JCN; c++)
            alpha = __fadd_rn(alpha, fabsf(__fsub_rn(j0[c], jt[c])));
        alpha = __fmul_rn(alpha, scale_index);
        const int idx = (int)alpha;
        alpha = __fsub_rn(alpha, (float)idx);
        const float l0 = lut[idx], l1 = lut[idx + 1];
        const float wgt = __fmul_rn(sw[k], __fadd_rn(l0, __fmul_rn(alpha, __fsub_rn(l1, l0))));
#pragma unroll
        for (int c = 0; c < SCN; c++)
            sum[c] = __fadd_rn(sum[c], __fmul_rn(wgt, st[c]));
        wsum = __fadd_rn(wsum, wgt);
    }
    const float inv = __fdiv_rn(1.0f, wsum);
#pragma unroll
    for (int c = 0; c < SCN; c++)
        dst[(img + (size_t)y * w + x) * SCN + c] = __fmul_rn(sum[c], inv);
}


// Register-tiled CV_32F kernel.  A float texel is 4*(JCN+SCN) bytes, so the (tile + 2r)^2 halo
// tile of the 8-bit kernels does not fit LDS for 3-channel images at the reference's radius; the
// texels therefore come through the vector cache, but each lane owns 4 horizontally adjacent
// outputs (one texel load feeds 4 outputs, lanes of a wave cover 64 contiguous pixels of 4 rows),
// the interpolated colour table and the spatial weight rows live in LDS, the spatial weights of a
// lane's 4 outputs slide through registers (one LDS read per column step), columns outside the
// disk carry weight 0 (adds +0 to the sums: the tap order per output is OpenCV's), and tiles
// away from the image border skip borderInterpolate.  Same float operations per tap as
// jbf_f32_kernel, so the values are identical.
// Tile height: 32 rows for every texel size.  (8 x 1080p, radius 33, with the four-column loop:
// 3/3-channel joint/src 328 / 449 / 459 MP/s with 16 / 32 / 64 rows, 3/1 342 / 560 / 574, 1/1 615 /
// 618 / 621.  With one column per iteration 16 rows had been the fastest for 6-float texels: the
// loads of more waves thrashed the vector cache without overlapping.)
constexpr int kF32TileW = 64;
constexpr int f32_tile_h(int, int) { return 32; }

// PAIR: the colour table arrives as pairs {lut[i], lut[i+1] - lut[i]} (lut_stride floats = lut_stride/2
// pairs per image, the last pair {0, 0}): one 8-byte LDS read per tap and output instead of two
// 4-byte ones at random addresses, and the table ends where its values reach zero (indices past
// the end are clamped to the last pair: weight 0 either way).  The difference is the float
// subtraction the plain form does per tap, done once per entry.
template <int JCN, int SCN, bool PAIR>
__global__ __launch_bounds__(16 * f32_tile_h(JCN, SCN)) void jbf_f32_quad_kernel(
    const float *__restrict__ joint, const float *__restrict__ src, float *__restrict__ dst, int h,
    int w, int border, const float *__restrict__ luts, int lut_stride,
    const float *__restrict__ scales, const float *__restrict__ swsym, int sw_len, int r4,
    int radius, const int *__restrict__ hwtab)
{
    extern __shared__ __align__(16) float f32_smem[];
    float *lut_s = f32_smem;                       // [lut_stride]
    float *sw_s = f32_smem + ((lut_stride + 3) & ~3);  // [(radius + 1) * sw_len]
    const int last_pair = lut_stride / 2 - 1;
    constexpr int kF32TileH = f32_tile_h(JCN, SCN), kF32Threads = 16 * kF32TileH;
    const int tid = threadIdx.x;
    {
        const float *lut = luts + (size_t)blockIdx.z * lut_stride;
        for (int i = tid; i < lut_stride; i += kF32Threads)
            lut_s[i] = lut[i];
        for (int i = tid; i < (radius + 1) * sw_len; i += kF32Threads)
            sw_s[i] = swsym[i];
    }
    __syncthreads();
    const int lx = tid & 15, ly = tid >> 4;
    const int tx0 = blockIdx.x * kF32TileW, ty0 = blockIdx.y * kF32TileH;
    const int x0 = tx0 + 4 * lx, y = min(ty0 + ly, h - 1);
    const size_t img = (size_t)blockIdx.z * h * w;
    const float scale_index = scales[blockIdx.z];
    // a tile whose taps all fall inside the image needs no border handling
    const bool interior = tx0 - r4 - 4 >= 0 && tx0 + kF32TileW + r4 + 8 <= w && ty0 - radius >= 0 &&
                          ty0 + kF32TileH + radius <= h;
    float j0[4][JCN];
#pragma unroll
    for (int p = 0; p < 4; p++) {
        const int xc = min(x0 + p, w - 1);
#pragma unroll
        for (int c = 0; c < JCN; c++)
            j0[p][c] = joint[(img + (size_t)y * w + xc) * JCN + c];
    }
    float sum[4][SCN], wsum[4];
#pragma unroll
    for (int p = 0; p < 4; p++) {
        wsum[p] = 0.f;
#pragma unroll
        for (int c = 0; c < SCN; c++)
            sum[p][c] = 0.f;
    }
    // One group of four columns c4 .. c4+3 of tap row (jrow, srow, wrow): the four texels are
    // requested together (their vector-cache latencies overlap), then consumed in tap order.
    // EDGE: the group straddles the end of some output's disk.  Columns of the span that lie off
    // output p's disk are not taps of p: OpenCV never reads them, so a NaN / Inf texel there must
    // not reach p (0 * Inf is NaN, and a NaN distance would index the table out of range); c, p
    // and hw are wave-uniform, the test is a scalar branch.  Groups inside every output's disk
    // (all but the first and last one or two of a row) run without it.
    auto group = [&](auto interior_c, auto edge_c, const float *jrow, const float *srow,
                     const float *wrow, int c4, int hw, float &w0, float &w1, float &w2, float &w3)
                     __attribute__((always_inline)) {
        constexpr bool INTERIOR = decltype(interior_c)::value, EDGE = decltype(edge_c)::value;
        float jt[4][JCN], st[4][SCN], wn[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int xx = INTERIOR ? x0 + c4 + u : border_interpolate(x0 + c4 + u, w, border);
#pragma unroll
            for (int ch = 0; ch < JCN; ch++)
                jt[u][ch] = jrow[(size_t)xx * JCN + ch];
#pragma unroll
            for (int ch = 0; ch < SCN; ch++)
                st[u][ch] = srow[(size_t)xx * SCN + ch];
            wn[u] = wrow[c4 + u + 1];
        }
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int c = c4 + u;
            const float ws[4] = {w0, w1, w2, w3};
#pragma unroll
            for (int p = 0; p < 4; p++) {
                if (EDGE && (c - p < -hw || c - p > hw))
                    continue;
                float alpha = 0.f;
#pragma unroll
                for (int ch = 0; ch < JCN; ch++)
                    alpha = __fadd_rn(alpha, fabsf(__fsub_rn(j0[p][ch], jt[u][ch])));
                alpha = __fmul_rn(alpha, scale_index);
                const int idx = (int)alpha;
                alpha = __fsub_rn(alpha, (float)idx);
                float l0, dl;
                if (PAIR) {
                    const float2 e = reinterpret_cast<const float2 *>(lut_s)[min(idx, last_pair)];
                    l0 = e.x;
                    dl = e.y;
                } else {
                    l0 = lut_s[idx];
                    dl = __fsub_rn(lut_s[idx + 1], l0);
                }
                const float wgt = __fmul_rn(ws[p], __fadd_rn(l0, __fmul_rn(alpha, dl)));
#pragma unroll
                for (int ch = 0; ch < SCN; ch++)
                    sum[p][ch] = __fadd_rn(sum[p][ch], __fmul_rn(wgt, st[u][ch]));
                wsum[p] = __fadd_rn(wsum[p], wgt);
            }
            w3 = w2;
            w2 = w1;
            w1 = w0;
            w0 = wn[u];
        }
    };
    auto rows = [&](auto interior_c) __attribute__((always_inline)) {
        constexpr bool INTERIOR = decltype(interior_c)::value;
        for (int i = -radius; i <= radius; i++) {
            const int hw = hwtab[i + radius];
            const int hw4 = (hw + 3) & ~3;
            const int yy = INTERIOR ? y + i : border_interpolate(y + i, h, border);
            const float *jrow = joint + (img + (size_t)yy * w) * JCN;
            const float *srow = src + (img + (size_t)yy * w) * SCN;
            // wrow[j], zero off the disk; the weights of outputs 0..3 at column step c are
            // wrow[c], wrow[c-1], wrow[c-2], wrow[c-3] and slide through registers
            const float *wrow = sw_s + (i < 0 ? -i : i) * sw_len + (r4 + 8);
            float w0 = wrow[-hw4], w1 = wrow[-hw4 - 1], w2 = wrow[-hw4 - 2], w3 = wrow[-hw4 - 3];
            for (int c4 = -hw4; c4 <= hw4; c4 += 4) {
                if (c4 - 3 >= -hw && c4 + 3 <= hw)
                    group(interior_c, std::false_type{}, jrow, srow, wrow, c4, hw, w0, w1, w2, w3);
                else
                    group(interior_c, std::true_type{}, jrow, srow, wrow, c4, hw, w0, w1, w2, w3);
            }
        }
    };
    if (interior)
        rows(std::true_type{});
    else
        rows(std::false_type{});
    if (ty0 + ly >= h)
        return;
#pragma unroll
    for (int p = 0; p < 4; p++) {
        if (x0 + p >= w)
            continue;
        const float inv = __fdiv_rn(1.0f, wsum[p]);
#pragma unroll
        for (int c = 0; c < SCN; c++)
            dst[(img + (size_t)y * w + x0 + p) * SCN + c] = __fmul_rn(sum[p][c], inv);
    }
}

}  // namespace

}  // namespace rf

extern "C" size_t rf_jbf_f32_workspace_bytes(int n, int joint_cn)
{
    if (n <= 0 || (joint_cn != 1 && joint_cn != 3))
        return 0;
    // room for the pair form of the table (jbf_f32_quad_kernel): two floats per entry
    const size_t lut = (size_t)(rf::kF32BinsPerChannel * joint_cn + 3) * 2 * sizeof(float);
    return (size_t)n * (lut + 2 * sizeof(uint32_t) + sizeof(float)) + 256;
}

extern "C" int rf_jbf_f32(const float *joint, const float *src, float *dst, int n, int h, int w,
                          int joint_cn, int src_cn, int d, double sigma_color, double sigma_space,
                          int border, void *workspace, size_t workspace_bytes, void *stream_)
{
    using namespace rf;
    if (n == 0)
        return RF_OK;
    if (!joint || !src || !dst || !workspace)
        return fail(RF_E_BADARG, "rf_jbf_f32: NULL pointer");
    if (n < 0 || h <= 0 || w <= 0)
        return fail(RF_E_BADARG, "rf_jbf_f32: bad size n=%d h=%d w=%d", n, h, w);
    if ((joint_cn != 1 && joint_cn != 3) || (src_cn != 1 && src_cn != 3))
        return fail(RF_E_UNSUPPORTED, "rf_jbf_f32: channels must be 1 or 3 (joint %d, src %d)",
                    joint_cn, src_cn);
    // BORDER_CONSTANT: the zero padding lies outside the joint's value range, so OpenCV's own
    // 32F code indexes its table out of bounds there (undefined); not offered
    if (border < 1 || border > 4)
        return fail(RF_E_UNSUPPORTED, "rf_jbf_f32: border type %d", border);
    {
        const size_t px = (size_t)n * h * w * sizeof(float);
        if (ranges_overlap(dst, px * src_cn, joint, px * joint_cn) ||
            ranges_overlap(dst, px * src_cn, src, px * src_cn))
            return fail(RF_E_BADARG, "rf_jbf_f32: dst must not overlap an input");
    }
    if (n > 65535)
        return fail(RF_E_UNSUPPORTED, "rf_jbf_f32: n <= 65535 per call");
    if (workspace_bytes < rf_jbf_f32_workspace_bytes(n, joint_cn))
        return fail(RF_E_WORKSPACE, "rf_jbf_f32: workspace %zu B < %zu B", workspace_bytes,
                    rf_jbf_f32_workspace_bytes(n, joint_cn));
    sigma_color = jbf_sigma(sigma_color);
    sigma_space = jbf_sigma(sigma_space);
    const int radius = jbf_radius(d, sigma_space);
    if (radius > kJbfMaxRadius)
        return fail(RF_E_UNSUPPORTED, "rf_jbf_f32: radius %d too large", radius);
    hipStream_t stream = (hipStream_t)stream_;
    // (before the tables and the first copy: a refused call leaves the capture as it found it)
    if (stream_is_capturing(stream))
        return fail(RF_E_UNSUPPORTED, "rf_jbf_f32: synchronises its stream and cannot be captured "
                                      "into a graph");
    JbfTables t;  // tap offsets and spatial weights are those of the 8-bit path
    TablesHold hold{t};
    int rc = get_tables(radius, joint_cn, sigma_color, sigma_space, stream, &t);
    if (rc != RF_OK)
        return rc;
    // workspace: [n] (min,max) ordered bits | [n] scale_index | [n] tables
    const int bins = kF32BinsPerChannel * joint_cn;
    uint32_t *d_minmax = reinterpret_cast<uint32_t *>(workspace);
    float *d_scale = reinterpret_cast<float *>(d_minmax + 2 * (size_t)n);
    float *d_luts = reinterpret_cast<float *>(
        static_cast<char *>(workspace) + (((size_t)n * 12 + 255) & ~(size_t)255));
    std::vector<uint32_t> mm(2 * (size_t)n);
    for (int i = 0; i < n; i++) {
        mm[2 * i] = 0xffffffffu;
        mm[2 * i + 1] = 0u;
    }
    RF_HIP_CHECK(hipMemcpyAsync(d_minmax, mm.data(), mm.size() * 4, hipMemcpyHostToDevice, stream));
    const size_t count = (size_t)h * w * joint_cn;
    const int mb = (int)std::min<size_t>(256, (count + 1023) / 1024);
    hipLaunchKernelGGL(jbf_f32_minmax_kernel, dim3(mb, n), dim3(256), 0, stream, joint, d_minmax,
                       count);
    // The table depends on the joint's value range and is built with the host's exp (the same
    // libm the CPU path uses), so the range comes back to the host: this entry point
    // synchronises the stream.
    RF_HIP_CHECK(hipMemcpyAsync(mm.data(), d_minmax, mm.size() * 4, hipMemcpyDeviceToHost, stream));
    RF_HIP_CHECK(hipStreamSynchronize(stream));
    std::vector<float> luts((size_t)n * (bins + 2)), scales(n);
    const double gauss_color_coeff = -0.5 / (sigma_color * sigma_color);
    for (int i = 0; i < n; i++) {
        const double minv = from_ordered_bits(mm[2 * i]), maxv = from_ordered_bits(mm[2 * i + 1]);
        if (std::fabs(minv - maxv) < FLT_EPSILON)
            return fail(RF_E_UNSUPPORTED, "rf_jbf_f32: image %d has a constant joint (OpenCV falls "
                        "back to a Gaussian blur there, which is not implemented)", i);
        const float len = (float)(maxv - minv) * joint_cn;
        const float scale_index = bins / len;
        scales[i] = scale_index;
        float *lut = luts.data() + (size_t)i * (bins + 2);
        float last = 1.f;
        for (int b = 0; b < bins + 2; b++) {
            if (last > 0.f) {
                const double val = b / scale_index;
                lut[b] = (float)std::exp(val * val * gauss_color_coeff);
                last = lut[b];
            } else {
                lut[b] = 0.f;
            }
        }
    }
    RF_HIP_CHECK(hipMemcpy(d_scale, scales.data(), scales.size() * 4, hipMemcpyHostToDevice));
    // register-tiled kernel when its LDS tables fit (always at the reference's radius); the
    // one-thread-per-pixel kernel otherwise, and as the cross-check (debug option jbf_f32_untiled)
    size_t quad_lds = (size_t)(((bins + 2 + 3) & ~3) + (radius + 1) * t.sw_len) * sizeof(float);
    const bool quad = quad_lds <= 64 * 1024 && !debug_get(kDbgJbfF32Untiled);
    // Pair form of the table (see jbf_f32_quad_kernel) when it fits LDS beside the weight rows: a
    // table that reaches zero ends there; z = first zero entry (every entry after it is zero by
    // construction)
    int lut_stride = bins + 2;
    bool pair = false;
    if (quad) {
        int zmax = 0;
        for (int i = 0; i < n; i++) {
            const float *lut = luts.data() + (size_t)i * (bins + 2);
            int z = 0;
            while (z < bins + 2 && lut[z] > 0.f)
                z++;
            zmax = std::max(zmax, z);
        }
        const int npair = zmax + 1;  // pairs 0 .. zmax; pair zmax = {0, 0}
        const size_t pair_lds =
            (size_t)(((2 * npair + 3) & ~3) + (radius + 1) * t.sw_len) * sizeof(float);
        if (npair <= bins + 3 && pair_lds <= 64 * 1024) {
            pair = true;
            lut_stride = 2 * npair;
            std::vector<float> pairs((size_t)n * lut_stride);
            for (int i = 0; i < n; i++) {
                const float *lut = luts.data() + (size_t)i * (bins + 2);
                float *pp = pairs.data() + (size_t)i * lut_stride;
                for (int b = 0; b < npair; b++) {
                    const float l0 = b < bins + 2 ? lut[b] : 0.f;
                    const float l1 = b + 1 < bins + 2 ? lut[b + 1] : 0.f;
                    pp[2 * b] = l0;
                    pp[2 * b + 1] = l1 - l0;
                }
            }
            luts.swap(pairs);
            quad_lds = (size_t)(((lut_stride + 3) & ~3) + (radius + 1) * t.sw_len) * sizeof(float);
        }
    }
    RF_HIP_CHECK(hipMemcpy(d_luts, luts.data(), luts.size() * 4, hipMemcpyHostToDevice));
    dim3 grid(ceil_div(w, 64), ceil_div(h, 4), n);
#define RF_F32(J_, S_)                                                                         \
    do {                                                                                       \
        if (quad && pair)                                                                      \
            hipLaunchKernelGGL((jbf_f32_quad_kernel<J_, S_, true>),                            \
                               dim3(ceil_div(w, kF32TileW), ceil_div(h, f32_tile_h(J_, S_)), n), \
                               dim3(16 * f32_tile_h(J_, S_)), quad_lds, stream, joint, src, dst, \
                               h, w, border, d_luts, lut_stride, d_scale, t.d_swsym, t.sw_len, \
                               t.r4, radius, t.d_hw);                                          \
        else if (quad)                                                                         \
            hipLaunchKernelGGL((jbf_f32_quad_kernel<J_, S_, false>),                           \
                               dim3(ceil_div(w, kF32TileW), ceil_div(h, f32_tile_h(J_, S_)), n), \
                               dim3(16 * f32_tile_h(J_, S_)), quad_lds, stream, joint, src, dst, \
                               h, w, border, d_luts, bins + 2, d_scale, t.d_swsym, t.sw_len,   \
                               t.r4, radius, t.d_hw);                                          \
        else                                                                                   \
            hipLaunchKernelGGL((jbf_f32_kernel<J_, S_>), grid, dim3(256), 0, stream, joint, src, \
                               dst, h, w, border, d_luts, bins + 2, d_scale, t.d_di, t.d_dj,   \
                               t.d_sw, t.maxk);                                                \
    } while (0)
    if (joint_cn == 3 && src_cn == 3)
        RF_F32(3, 3);
    else if (joint_cn == 3)
        RF_F32(3, 1);
    else if (src_cn == 3)
        RF_F32(1, 3);
    else
        RF_F32(1, 1);
#undef RF_F32
    RF_HIP_CHECK(hipGetLastError());
    return RF_OK;
}
