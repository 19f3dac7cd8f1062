// rf_train_hinge.hip -- WHDR hinge loss and its gradient at de-duplicated judgement points.
//
// Restates the reference's training/layers/whdr_hinge_loss_layer.py:126-230 (lightness of one
// channel: whdr_layer.py:179-198) over the arrays of whdr.dedup_points plus a point incidence list
// (train.point_incidence).  One workgroup of 256 per image: first the image's weighted loss and weight
// sum (256 strided float64 partial sums, then a fixed pairwise tree), then one thread per point walks
// the point's incidence list and re-evaluates each of its comparisons.  Sum orders: the header.
#include <cfloat>
#include <cmath>

#include "rf_train_common.hpp"

namespace rft {
namespace {

constexpr int kHingeThreads = 256;

// the four borders, formed in double on the host and rounded to float32 (the reference compares a
// float32 ratio with a Python float, which NumPy >= 2 rounds to float32 first)
struct Borders {
    float dark1;       // 1 / (1 + delta + margin)
    float dark2;       // 1 + delta + margin
    float equal;       // 1 + delta - margin
    float equal_inv;   // 1 / (1 + delta - margin)
    int wide_margin;   // margin > delta
};

// One comparison, unweighted: the loss term and the two products dl/dy * dy/dL1, dl/dy * dy/dL2.
__device__ __forceinline__ void eval_comparison(float r1, float r2, int darker, const Borders &b,
                                                float &loss, float &g1, float &g2)
{
    const float l1 = fmaxf(FLT_EPSILON, r1), l2 = fmaxf(FLT_EPSILON, r2);
    const float l2inv = __fdiv_rn(1.0f, l2);
    const float y = __fmul_rn(l1, l2inv);
    const float dy1 = l2inv, dy2 = __fmul_rn(-y, l2inv);
    float dldy = 0.f;
    loss = 0.f;
    if (darker == 1) {
        if (y > b.dark1) {
            loss = __fsub_rn(y, b.dark1);
            dldy = 1.f;
        }
    } else if (darker == 2) {
        if (y < b.dark2) {
            loss = __fsub_rn(b.dark2, y);
            dldy = -1.f;
        }
    } else if (darker == 0) {
        if (!b.wide_margin) {
            if (y > b.equal) {
                loss = __fsub_rn(y, b.equal);
                dldy = 1.f;
            } else if (y < b.equal_inv) {
                loss = __fsub_rn(b.equal_inv, y);
                dldy = -1.f;
            }
        } else {
            loss = fmaxf(__fsub_rn(b.equal_inv, y), __fsub_rn(y, b.equal));
            dldy = y > 1.f ? 1.f : -1.f;
        }
    }
    g1 = __fmul_rn(dldy, dy1);
    g2 = __fmul_rn(dldy, dy2);
}

__global__ __launch_bounds__(kHingeThreads) void whdr_hinge_points_kernel(
    const float *__restrict__ r, const int *__restrict__ point_offsets,
    const int *__restrict__ comps, const double *__restrict__ weights,
    const int *__restrict__ comp_offsets, const int *__restrict__ inc_offsets,
    const int *__restrict__ inc, int n, Borders b, double *__restrict__ loss_out,
    float *__restrict__ grad_r)
{
    __shared__ double s_loss[kHingeThreads];
    __shared__ double s_wsum[kHingeThreads];
    const int img = blockIdx.x, t = threadIdx.x;
    const int p0 = point_offsets[img], p1 = point_offsets[img + 1];
    const int k0 = comp_offsets[img], k1 = comp_offsets[img + 1];
    const float *rp = r + p0;

    double loss = 0.0, wsum = 0.0;
    for (int k = k0 + t; k < k1; k += kHingeThreads) {
        const int *c = comps + (size_t)k * 3;
        const double w = weights[k];
        float l, g1, g2;
        eval_comparison(rp[c[0]], rp[c[1]], c[2], b, l, g1, g2);
        loss += w * (double)l;
        wsum += w;
    }
    s_loss[t] = loss;
    s_wsum[t] = wsum;
    __syncthreads();
    for (int s = kHingeThreads / 2; s > 0; s >>= 1) {
        if (t < s) {
            s_loss[t] += s_loss[t + s];
            s_wsum[t] += s_wsum[t + s];
        }
        __syncthreads();
    }
    const double total_w = s_wsum[0];
    if (t == 0)
        loss_out[img] = total_w != 0.0 ? s_loss[0] / total_w : 0.0;

    for (int p = p0 + t; p < p1; p += kHingeThreads) {
        double g = 0.0;
        if (total_w != 0.0) {
            const int e0 = inc_offsets[p], e1 = inc_offsets[p + 1];
            for (int e = e0; e < e1; e++) {
                const int entry = inc[e];
                const int k = k0 + (entry >> 1);
                const int *c = comps + (size_t)k * 3;
                float l, g1, g2;
                eval_comparison(rp[c[0]], rp[c[1]], c[2], b, l, g1, g2);
                g += weights[k] * (double)((entry & 1) ? g2 : g1);
            }
            g = g / total_w / (double)n;
        }
        grad_r[p] = (float)g;
    }
}

}  // namespace
}  // namespace rft

extern "C" int rf_train_whdr_hinge_points_f32(const float *r, const int *point_offsets,
                                              const int *comps, const double *weights,
                                              const int *comp_offsets, const int *inc_offsets,
                                              const int *inc, int n, double delta, double margin,
                                              double *loss_out, float *grad_r, void *stream_)
{
    using namespace rft;
    const char *who = "rf_train_whdr_hinge_points_f32";
    if (n == 0)  // an empty batch is valid whatever the (possibly NULL) pointers are
        return kOk;
    if (n < 0)
        return fail(kBadArg, "%s: bad size n=%d", who, n);
    if (!r || !point_offsets || !comps || !weights || !comp_offsets || !inc_offsets || !inc ||
        !loss_out || !grad_r)
        return fail(kBadArg, "%s: NULL pointer", who);
    if (!(delta >= 0) || !std::isfinite(delta))
        return fail(kBadArg, "%s: delta must be finite and >= 0", who);
    if (!(margin >= 0) || !std::isfinite(margin))
        return fail(kBadArg, "%s: margin must be finite and >= 0", who);
    // a workgroup per image: gridDim x blockDim stays below 2^32 work-items
    if ((unsigned long long)n * kHingeThreads >= (1ull << 32))
        return fail(kUnsupported, "%s: too many images for one launch", who);
    Borders b;
    b.dark1 = (float)(1.0 / (1.0 + delta + margin));
    b.dark2 = (float)(1.0 + delta + margin);
    b.equal = (float)(1.0 + delta - margin);
    b.equal_inv = (float)(1.0 / (1.0 + delta - margin));
    b.wide_margin = margin > delta;
    hipLaunchKernelGGL(whdr_hinge_points_kernel, dim3((unsigned)n), dim3(kHingeThreads), 0,
                       (hipStream_t)stream_, r, point_offsets, comps, weights, comp_offsets,
                       inc_offsets, inc, n, b, loss_out, grad_r);
    RFT_HIP_CHECK(hipGetLastError());
    return kOk;
}
