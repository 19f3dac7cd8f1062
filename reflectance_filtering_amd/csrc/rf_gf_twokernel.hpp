// rf_gf_twokernel.hpp -- the two-kernel stage 2 of the guided filter: RowSum<float,double> and
// ColumnSum<double,float> as a kernel pair that writes every double row sum (radius 0, the debug option
// "gf_two_kernel", and every box filter of the float path).  Included by rf_gf.hip, which instantiates
// gf_rowsum_kernel<4> and gf_colsum_apply_kernel<3,3> / <1,3> / <1,1>, and by rf_gf_f32.hip, which
// instantiates gf_rowsum_kernel<1> and gf_colsum_apply_kernel<SCN,SCN,float>: disjoint sets, so every
// kernel is compiled in one unit.
#pragma once
#include "rf_gf_fused.hpp"

namespace rf {
namespace {

// ------------------------------------------------------------------------------------------
// stage 2a: RowSum<float,double>.  One wave = 64 rows of one plane, one lane per row, walking
// the border-extended row left to right; tiles are transposed through LDS so that global
// loads/stores stay row-contiguous.
// ------------------------------------------------------------------------------------------
constexpr int kBChunk = 32;

// planes: [img][src_np][h][w] (il = 1) or [img][src_np / 4][h][w][4] (il = 4: groups of four
// planes interleaved per pixel, the layout stage 1 writes), of which the first np per image are
// summed; rowsums: [img][np][h][w]
template <int il>
__global__ __launch_bounds__(64) void gf_rowsum_kernel(const float *__restrict__ planes,
                                                       double *__restrict__ rowsums, int h, int w,
                                                       int radius, int row_blocks, int np,
                                                       const int *__restrict__ colour, int src_np)
{
    {
        // grey 3-channel images only carry the 4 planes of their first channel
        const int pl = blockIdx.x / row_blocks;
        if (colour != nullptr && pl % np >= 4 && colour[pl / np] == 0)
            return;
    }
    __shared__ float t_in[kBRows][kBChunk + 1];
    __shared__ float t_out_lo[kBRows][kBChunk + 1];  // leaving values
    __shared__ double t_d[kBRows][kBChunk + 1];

    const int lane = threadIdx.x;
    const int plane = blockIdx.x / row_blocks;  // plane index across the whole chunk of images
    const int row0 = (blockIdx.x - plane * row_blocks) * kBRows;
    const int q = plane % np;  // plane of the image
    const float *S = planes + ((size_t)(plane / np) * src_np + q / il * il) * h * w + q % il;
    double *D = rowsums + (size_t)plane * h * w;
    const int ks = 2 * radius + 1;
    const int sub = lane >> 5, col = lane & 31;  // loader role: 2 rows x 32 columns per instruction

    double s = 0.0;
    // prologue: s = sum_{i<ks} ext[i], ext[i] = S[bi(i - r)]
    for (int i0 = 0; i0 < ks; i0 += kBChunk) {
        const int xi = i0 + col;
        const int sx = border_interpolate(min(xi, ks - 1) - radius, w, RF_BORDER_REFLECT);
        for (int rr = 0; rr < kBRows; rr += 2) {
            const int row = min(row0 + rr + sub, h - 1);
            t_in[rr + sub][col] = S[((size_t)row * w + sx) * il];
        }
        __syncthreads();
        const int cnt = min(kBChunk, ks - i0);
        for (int c = 0; c < cnt; c++)
            s += (double)t_in[lane][c];
        __syncthreads();
    }
    // D[0] = s; then D[o] for o = 1..w-1:  s += (double)ext[o-1+ks] - (double)ext[o-1]
    // chunk over o in [1, w): entering S[bi(o + r)], leaving S[bi(o - 1 - r)]
    for (int o0 = 0; o0 < w; o0 += kBChunk) {
        const int o = o0 + col;
        const int se = border_interpolate(min(o, w - 1) + radius, w, RF_BORDER_REFLECT);
        const int sl = border_interpolate(min(o, w - 1) - 1 - radius, w, RF_BORDER_REFLECT);
        for (int rr = 0; rr < kBRows; rr += 2) {
            const int row = min(row0 + rr + sub, h - 1);
            t_in[rr + sub][col] = S[((size_t)row * w + se) * il];
            t_out_lo[rr + sub][col] = S[((size_t)row * w + sl) * il];
        }
        __syncthreads();
        const int cnt = min(kBChunk, w - o0);
        for (int c = 0; c < cnt; c++) {
            if (o0 + c > 0)
                s += (double)t_in[lane][c] - (double)t_out_lo[lane][c];
            t_d[lane][c] = s;
        }
        __syncthreads();
        if (o < w)
            for (int rr = 0; rr < kBRows; rr += 2) {
                const int row = row0 + rr + sub;
                if (row < h)
                    D[(size_t)row * w + o] = t_d[rr + sub][col];
            }
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------
// stage 2b: ColumnSum<double,float> + ApplyTransform + convertTo(uint8).
// block = 64 columns x (4*SCN) planes; every thread walks its column of one plane from the
// top of the image; per output row the 4 means of a src channel meet in LDS and the beta
// thread of that channel forms q = beta + a0*I0 + a1*I1 + a2*I2 and stores the byte.
// ------------------------------------------------------------------------------------------
// T = uint8_t (result rounded and saturated) or float (the CV_32F variant: result stored as is)
// gcn: guide values per pixel, 3, or 1 for a grey guide standing for three equal channels
template <int SCN, int SPX, typename T = uint8_t>
__global__ __launch_bounds__(64 * 4 * SCN) void gf_colsum_apply_kernel(
    const double *__restrict__ rowsums, const T *__restrict__ guide, T *__restrict__ dst, int h,
    int w, int radius, const int *__restrict__ colour, int gcn)
{
    if (wrong_variant<SCN>(colour, blockIdx.z))
        return;
    constexpr int NP = 4 * SCN;
    constexpr int kDepth = 4;
    __shared__ float means[2][NP][64];

    const int lane = threadIdx.x;
    const int plane = threadIdx.y;
    const int x = blockIdx.x * 64 + lane;
    const int xc = min(x, w - 1);
    const size_t npx = (size_t)h * w;
    const double *R = rowsums + ((size_t)blockIdx.z * (4 * SPX) + plane) * npx + xc;
    const T *gimg = guide + (size_t)blockIdx.z * npx * gcn;
    T *dimg = dst + (size_t)blockIdx.z * npx * SPX;
    const int gstep = gcn == 3 ? 1 : 0;  // a grey guide's one value serves all three channels
    const int ks = 2 * radius + 1;
    const double scale = 1.0 / (double)(ks * ks);

    double SUM = 0.0;
    for (int yy = -radius; yy < radius; yy++)
        SUM += R[(size_t)border_interpolate(yy, h, RF_BORDER_REFLECT) * w];

    for (int y0 = 0; y0 < h; y0 += kDepth) {
        double sp[kDepth], sm[kDepth];
#pragma unroll
        for (int k = 0; k < kDepth; k++) {
            const int y = min(y0 + k, h - 1);
            sp[k] = R[(size_t)border_interpolate(y + radius, h, RF_BORDER_REFLECT) * w];
            sm[k] = R[(size_t)border_interpolate(y - radius, h, RF_BORDER_REFLECT) * w];
        }
#pragma unroll
        for (int k = 0; k < kDepth; k++) {
            const int y = y0 + k;
            if (y >= h)
                break;
            const double s0 = SUM + sp[k];
            means[y & 1][plane][lane] = (float)(s0 * scale);
            SUM = s0 - sm[k];
            __syncthreads();
            if ((plane & 3) == 3 && x < w) {
                const int s = plane >> 2;
                const size_t pix = (size_t)y * w + x;
                float q = means[y & 1][plane][lane];
#pragma unroll
                for (int g = 0; g < 3; g++)
                    q = __fadd_rn(q, __fmul_rn(means[y & 1][s * 4 + g][lane],
                                               (float)gimg[pix * gcn + g * gstep]));
                T o;
                if constexpr (sizeof(T) == 1)
                    o = saturate_u8(q);
                else
                    o = q;
                if (SCN == SPX) {
                    dimg[pix * SCN + s] = o;
                } else {  // grey image: the one computed channel stands for all three
                    dimg[pix * 3 + 0] = o;
                    dimg[pix * 3 + 1] = o;
                    dimg[pix * 3 + 2] = o;
                }
            }
        }
    }
}

}  // namespace
}  // namespace rf
