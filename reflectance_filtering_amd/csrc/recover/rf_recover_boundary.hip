// rf_recover_boundary.hip -- both boundary losses over every pixel of a run and their gradient
// towards the network output, through the recover layer.
//
// Restates the reference's training/layers/boundary_loss_layer.py on the two tops of
// recover_reflectance_shading_layer.py and that layer's backward pass (np.sum over the six channels).
// A workgroup of 256 stages the 768 dwords of 256 interleaved pixels through LDS (lane-contiguous
// dword loads; a run may start at any 4-byte boundary), then one thread per pixel.  The per-pixel
// float32 losses are summed in float64: per thread over its passes, a fixed pairwise tree per
// workgroup, and the workgroups' rows by a second kernel (orders: the header).
#include "rf_recover_common.hpp"

namespace rfr {
namespace {

constexpr int kMaxWgs = 1024;   // four workgroups for each of the 256 CUs

// loss and slope of one blob's intensity v
__device__ __forceinline__ void boundary_term(float v, int penalty, float &loss, float &slope)
{
    loss = 0.f;
    slope = 0.f;
    if (penalty == RF_RECOVER_PENALTY_L1) {
        if (v < 0.f) {
            loss = -v;
            slope = -1.f;
        } else if (v > 1.f) {
            loss = __fsub_rn(v, 1.0f);
            slope = 1.f;
        }
    } else {
        if (v < 0.f) {
            loss = __fmul_rn(v, v);
            slope = __fmul_rn(2.0f, v);
        } else if (v > 1.f) {
            const float t = __fsub_rn(v, 1.0f);
            loss = __fmul_rn(t, t);
            slope = __fmul_rn(2.0f, t);
        }
    }
}

__global__ __launch_bounds__(kThreads) void boundary_backward_kernel(
    const float *__restrict__ x, const float *__restrict__ e, int npixels, int passes, int norm,
    int penalty, float scale_r, float scale_s, double *__restrict__ partial,
    float *__restrict__ grad_e)
{
    __shared__ float s_x[3 * kThreads];
    __shared__ double s_r[kThreads];
    __shared__ double s_s[kThreads];
    const int t = threadIdx.x;
    const float count = (float)npixels;
    double sum_r = 0.0, sum_s = 0.0;
    for (int pass = blockIdx.x; pass < passes; pass += gridDim.x) {
        const size_t base = (size_t)pass * kThreads;
        const int rest = npixels - (int)base;
        const int live = rest < kThreads ? rest : kThreads;
        const float *src = x + 3 * base;
        for (int i = t; i < 3 * live; i += kThreads)
            s_x[i] = src[i];
        __syncthreads();
        if (t < live) {
            const Pixel p = recover_pixel(s_x[3 * t], s_x[3 * t + 1], s_x[3 * t + 2], e[base + t], norm);
            float loss_r, slope_r, loss_s, slope_s;
            boundary_term(mean3(p.refl[0], p.refl[1], p.refl[2]), penalty, loss_r, slope_r);
            boundary_term(mean3(p.s, p.s, p.s), penalty, loss_s, slope_s);
            const float dr = __fmul_rn(__fdiv_rn(__fdiv_rn(slope_r, count), 3.0f), scale_r);
            const float ds = __fmul_rn(__fdiv_rn(__fdiv_rn(slope_s, count), 3.0f), scale_s);
            float g = __fadd_rn(__fmul_rn(dr, p.n[0]), __fmul_rn(dr, p.n[1]));
            g = __fadd_rn(g, __fmul_rn(dr, p.n[2]));
            const float shade = __fmul_rn(ds, p.ds);
            g = __fadd_rn(__fadd_rn(__fadd_rn(g, shade), shade), shade);
            grad_e[base + t] = g;
            sum_r += (double)loss_r;
            sum_s += (double)loss_s;
        }
        __syncthreads();
    }
    s_r[t] = sum_r;
    s_s[t] = sum_s;
    __syncthreads();
    for (int w = kThreads / 2; w > 0; w >>= 1) {
        if (t < w) {
            s_r[t] += s_r[t + w];
            s_s[t] += s_s[t + w];
        }
        __syncthreads();
    }
    if (t == 0) {
        partial[2 * (size_t)blockIdx.x] = s_r[0];
        partial[2 * (size_t)blockIdx.x + 1] = s_s[0];
    }
}

__global__ void boundary_reduce_kernel(const double *__restrict__ partial, int rows, int npixels,
                                       double *__restrict__ loss_out)
{
    const int j = threadIdx.x;
    if (j >= 2)
        return;
    double sum = 0.0;
    for (int g = 0; g < rows; g++)
        sum += partial[2 * (size_t)g + j];
    loss_out[j] = sum / (double)npixels;
}

struct Plan {
    int passes, workgroups;
    size_t bytes;
};

int make_plan(const char *who, long long npixels, Plan *plan)
{
    if (int bad = check_sizes(who, npixels, 0))
        return bad;
    plan->passes = (int)((npixels + kThreads - 1) / kThreads);
    plan->workgroups = plan->passes < kMaxWgs ? plan->passes : kMaxWgs;
    plan->bytes = ((size_t)plan->workgroups * 2 * sizeof(double) + 15) & ~(size_t)15;
    return kOk;
}

}  // namespace
}  // namespace rfr

extern "C" size_t rf_recover_boundary_workspace_bytes(long long npixels)
{
    rfr::Plan plan;
    if (rfr::make_plan("rf_recover_boundary_workspace_bytes", npixels, &plan) != rfr::kOk)
        return 0;
    return plan.bytes;
}

extern "C" int rf_recover_boundary_plan(long long npixels, int out[3])
{
    using namespace rfr;
    if (!out)
        return fail(kBadArg, "rf_recover_boundary_plan: NULL pointer");
    Plan plan;
    if (int bad = make_plan("rf_recover_boundary_plan", npixels, &plan))
        return bad;
    out[0] = kThreads;
    out[1] = plan.workgroups;
    out[2] = plan.workgroups;
    return kOk;
}

extern "C" int rf_recover_boundary_backward_f32(const float *x, const float *e, long long npixels,
                                                int norm, int penalty, float scale_reflectance,
                                                float scale_shading, double *loss_out,
                                                float *grad_e, void *workspace,
                                                size_t workspace_bytes, void *stream_)
{
    using namespace rfr;
    const char *who = "rf_recover_boundary_backward_f32";
    Plan plan;
    if (int bad = make_plan(who, npixels, &plan))
        return bad;
    hipStream_t stream = (hipStream_t)stream_;
    if (npixels == 0) {  // no pixels: valid whatever the other pointers are; an empty mean is 0
        if (loss_out)
            RFR_HIP_CHECK(hipMemsetAsync(loss_out, 0, 2 * sizeof(double), stream));
        return kOk;
    }
    if (!x || !e || !loss_out || !grad_e)
        return fail(kBadArg, "%s: NULL pointer", who);
    if (int bad = check_norm(who, norm))
        return bad;
    if (penalty != RF_RECOVER_PENALTY_L1 && penalty != RF_RECOVER_PENALTY_L2)
        return fail(kBadArg, "%s: unknown penalty %d (1 L1, 2 L2)", who, penalty);
    if (!std::isfinite(scale_reflectance) || !std::isfinite(scale_shading))
        return fail(kBadArg, "%s: the scales must be finite", who);
    if (!workspace || workspace_bytes < plan.bytes || ((uintptr_t)workspace & 15))
        return fail(kBadArg, "%s: workspace of %zu bytes, %zu needed (16-byte aligned)", who,
                    workspace ? workspace_bytes : (size_t)0, plan.bytes);
    double *partial = (double *)workspace;
    hipLaunchKernelGGL(boundary_backward_kernel, dim3((unsigned)plan.workgroups), dim3(kThreads), 0,
                       stream, x, e, (int)npixels, plan.passes, norm, penalty, scale_reflectance,
                       scale_shading, partial, grad_e);
    RFR_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(boundary_reduce_kernel, dim3(1), dim3(64), 0, stream,
                       (const double *)partial, plan.workgroups, (int)npixels, loss_out);
    RFR_HIP_CHECK(hipGetLastError());
    return kOk;
}
