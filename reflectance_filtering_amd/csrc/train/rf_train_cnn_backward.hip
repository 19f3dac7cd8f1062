// rf_train_cnn_backward.hip -- weight gradient of the shipped 1x1 reflectance CNN at P points.
//
//   x -> h0 = relu(W0 x + b0); h_l = relu(W_l h_{l-1} + b_l), l = 1..4; z = wf . [h0|..|h4] + bf;
//   r = 1 / (1 + exp(-z));   grad_w = d/dw sum_p grad_r[p] r(x_p; w)
//
// Form: lane = point for the forward and the delta passes, the weight-matrix gradients through the
// exact-f32 matrix instruction.  A workgroup is ONE wave and a pass is 64 consecutive points:
//   forward   every dot product is the float32 FMA chain of rf_cnn.hip (k ascending from 0, then
//             + bias), its weights wave-uniform scalar loads; the 160 post-ReLU activations of the
//             lane's point go to LDS as act[channel][point] (pitch 65: a column per lane for the
//             forward, a conflict-free row walk for the matrix operands)
//   delta     dz = grad_r r (1 - r); delta_l = relu'(h_l) * (W_{l+1}^T delta_{l+1} + dz wf_l),
//             written to LDS as dlt[channel][point]
//   dW_l      += delta_l (32 x 64 points) x h_{l-1}^T (64 points x 32): 32 steps of
//             v_mfma_f32_32x32x2_f32, A = dlt[lane & 31][p0 + (lane >> 5)],
//             B = act[32 (l-1) + (lane & 31)][p0 + (lane >> 5)]; the 32 x 32 sum stays in 16
//             accumulator registers per lane and layer over all passes of the workgroup
//   db_l, dW0 lanes 0..31 (channel = lane) sum dlt[channel][0..63] (and its products with the three
//             inputs for layer 0); lanes 32..63 (k = lane - 32) sum dz[p] * act[32 l + k][p]: dwf;
//             these sums are float64, point by point ascending, over all passes of the workgroup
// After its passes the workgroup writes its 4,513 sums as one float64 row of the workspace, and a
// second kernel adds the rows in float64, ascending.  Points past P in the last pass run with grad_r = 0
// on the inputs of point P - 1: every delta of theirs is exactly 0.
#include "rf_train_common.hpp"

namespace rft {
namespace {

typedef float float16v __attribute__((ext_vector_type(16)));

constexpr int kNP = RF_TRAIN_CNN_NPARAMS;
constexpr int kPts = 64;       // points per workgroup pass (one wave, lane = point)
constexpr int kPitch = 65;     // floats per LDS row
constexpr int kMaxWgs = 512;   // partial-gradient rows at most: two waves for each of the 256 CUs
constexpr int kWfOff = 128 + 4 * 1056, kBfOff = kNP - 1;

struct Lds {
    float act[160][kPitch];
    float dlt[32][kPitch];
    float xin[3][kPitch];
    float dz[kPitch];
    double dzd[kPts];  // grad_r * sigma' before its rounding to float: the bias and fuse-weight sums use it
};

// One 32-input layer forward for the lane's point: in = h_{l-1}, out to act[32 l + o][lane]; adds the
// layer's 32 terms of the fuse dot product to z in channel order.
__device__ __forceinline__ void forward_layer32(const float *__restrict__ wl,
                                                const float *__restrict__ wf_l, int l, Lds &s,
                                                int lane, float &z)
{
    float in[32];
#pragma unroll
    for (int k = 0; k < 32; k++)
        in[k] = s.act[32 * (l - 1) + k][lane];
#pragma unroll 2
    for (int o = 0; o < 32; o++) {
        const float *wo = wl + o * 32;
        float acc = 0.f;
#pragma unroll
        for (int k = 0; k < 32; k++)
            acc = __fmaf_rn(wo[k], in[k], acc);
        const float h = fmaxf(__fadd_rn(acc, wl[1024 + o]), 0.f);
        s.act[32 * l + o][lane] = h;
        z = __fmaf_rn(wf_l[o], h, z);
    }
}

// The sums over the 64 points of the pass that one lane owns: lanes 0..31 the bias gradient of
// channel `lane` (eb), lanes 32..63 the fuse-weight gradient of channel lane - 32 (ef).
// These sums are float64 (products of two floats are exact in it): a sequential float32 sum over
// the points loses more than the per-point arithmetic does.
__device__ __forceinline__ void point_sums(int l, const Lds &s, int lane, double &eb, double &ef)
{
    if (lane < 32) {
        double sum = eb;
#pragma unroll 8
        for (int p = 0; p < kPts; p++)
            sum += (double)s.dlt[lane][p];
        eb = sum;
    } else {
        double sum = ef;
#pragma unroll 8
        for (int p = 0; p < kPts; p++)
            sum = fma(s.dzd[p], (double)s.act[32 * l + lane - 32][p], sum);
        ef = sum;
    }
}

// Layer l = 4..1 backward: dlt holds delta_l on entry and delta_{l-1} on exit.
__device__ __forceinline__ void backward_layer32(const float *__restrict__ wl,
                                                 const float *__restrict__ wf_prev, int l, Lds &s,
                                                 int lane, float dz, float16v &acc_w, double &eb,
                                                 double &ef)
{
    __syncthreads();  // delta_l of every point is in dlt
    const int row = lane & 31, half = lane >> 5;
#pragma unroll 4
    for (int p0 = 0; p0 < kPts; p0 += 2)
        acc_w = __builtin_amdgcn_mfma_f32_32x32x2f32(s.dlt[row][p0 + half],
                                                     s.act[32 * (l - 1) + row][p0 + half], acc_w, 0,
                                                     0, 0);
    point_sums(l, s, lane, eb, ef);
    // W_l^T delta_l for the lane's point: c ascending, one row of W_l per step
    float prev[32];
#pragma unroll
    for (int k = 0; k < 32; k++)
        prev[k] = 0.f;
#pragma unroll 2
    for (int c = 0; c < 32; c++) {
        const float d = s.dlt[c][lane];
        const float *wc = wl + c * 32;
#pragma unroll
        for (int k = 0; k < 32; k++)
            prev[k] = __fmaf_rn(wc[k], d, prev[k]);
    }
    __syncthreads();  // every read of delta_l is done
#pragma unroll
    for (int k = 0; k < 32; k++) {
        const float g = __fmaf_rn(dz, wf_prev[k], prev[k]);
        s.dlt[k][lane] = s.act[32 * (l - 1) + k][lane] > 0.f ? g : 0.f;
    }
}

__global__ __launch_bounds__(kPts) void cnn_points_backward_kernel(
    const float *__restrict__ x, const float *__restrict__ w, const float *__restrict__ grad_r,
    int npoints, int passes, double *__restrict__ partial)
{
    __shared__ Lds s;
    const int lane = threadIdx.x;
    const float *wf = w + kWfOff;
    float16v acc_w[4];
#pragma unroll
    for (int l = 0; l < 4; l++)
#pragma unroll
        for (int j = 0; j < 16; j++)
            acc_w[l][j] = 0.f;
    double eb[5] = {0.0, 0.0, 0.0, 0.0, 0.0}, ef[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    double ew0[3] = {0.0, 0.0, 0.0};
    double dz_sum = 0.0;

    for (int pass = blockIdx.x; pass < passes; pass += gridDim.x) {
        const long long p = (long long)pass * kPts + lane;
        const bool live = p < npoints;
        const float *px = x + (size_t)(live ? p : npoints - 1) * 3;
        const float v[3] = {px[2], px[1], px[0]};  // the blob's channel order is R, G, B
        const float gr = live ? grad_r[p] : 0.f;
        __syncthreads();  // the previous pass has read all it needs of the LDS
#pragma unroll
        for (int k = 0; k < 3; k++)
            s.xin[k][lane] = v[k];
        float z = 0.f;
#pragma unroll 4
        for (int o = 0; o < 32; o++) {
            float acc = 0.f;
#pragma unroll
            for (int k = 0; k < 3; k++)
                acc = __fmaf_rn(w[o * 3 + k], v[k], acc);
            const float h = fmaxf(__fadd_rn(acc, w[96 + o]), 0.f);
            s.act[o][lane] = h;
            z = __fmaf_rn(wf[o], h, z);
        }
#pragma unroll 1
        for (int l = 1; l < 5; l++)
            forward_layer32(w + 128 + (l - 1) * 1056, wf + 32 * l, l, s, lane, z);
        const float zz = __fadd_rn(z, w[kBfOff]);
        // sigma'(z) = r (1 - r) formed in double from the float32 z of the forward chains: in float32,
        // 1 - r alone loses up to 2^-24 / (1 - r) of its value for a reflectance near 1
        const double rd = 1.0 / (1.0 + exp((double)(-zz)));
        const double dzd = (double)gr * (rd * (1.0 - rd));
        const float dz = (float)dzd;
        s.dzd[lane] = dzd;
        s.dz[lane] = dz;
        dz_sum += dzd;
#pragma unroll
        for (int c = 0; c < 32; c++)
            s.dlt[c][lane] = s.act[128 + c][lane] > 0.f ? __fmul_rn(dz, wf[128 + c]) : 0.f;

        backward_layer32(w + 128 + 3 * 1056, wf + 96, 4, s, lane, dz, acc_w[3], eb[4], ef[4]);
        backward_layer32(w + 128 + 2 * 1056, wf + 64, 3, s, lane, dz, acc_w[2], eb[3], ef[3]);
        backward_layer32(w + 128 + 1 * 1056, wf + 32, 2, s, lane, dz, acc_w[1], eb[2], ef[2]);
        backward_layer32(w + 128 + 0 * 1056, wf + 0, 1, s, lane, dz, acc_w[0], eb[1], ef[1]);
        __syncthreads();  // delta_0 of every point is in dlt
        if (lane < 32) {
            double sb = eb[0], s0 = ew0[0], s1 = ew0[1], s2 = ew0[2];
#pragma unroll 4
            for (int q = 0; q < kPts; q++) {
                const double d = (double)s.dlt[lane][q];
                sb += d;
                s0 = fma(d, (double)s.xin[0][q], s0);
                s1 = fma(d, (double)s.xin[1][q], s1);
                s2 = fma(d, (double)s.xin[2][q], s2);
            }
            eb[0] = sb, ew0[0] = s0, ew0[1] = s1, ew0[2] = s2;
        } else {
            double sum = ef[0];
#pragma unroll 8
            for (int q = 0; q < kPts; q++)
                sum = fma(s.dzd[q], (double)s.act[lane - 32][q], sum);
            ef[0] = sum;
        }
    }

    // the workgroup's row: every one of its 4,513 floats is written
    double *row = partial + (size_t)blockIdx.x * kNP;
#pragma unroll
    for (int l = 1; l < 5; l++) {
        double *wrow = row + 128 + (l - 1) * 1056;
#pragma unroll
        for (int j = 0; j < 16; j++) {
            const int c = (j & 3) + 8 * (j >> 2) + 4 * (lane >> 5);  // C/D map of the 32x32 tile
            wrow[c * 32 + (lane & 31)] = acc_w[l - 1][j];
        }
        if (lane < 32)
            wrow[1024 + lane] = eb[l];
        else
            row[kWfOff + 32 * l + lane - 32] = ef[l];
    }
    if (lane < 32) {
        row[96 + lane] = eb[0];
#pragma unroll
        for (int k = 0; k < 3; k++)
            row[lane * 3 + k] = ew0[k];
    } else {
        row[kWfOff + lane - 32] = ef[0];
    }
    // the lanes' sums of dz, added in lane order
    __syncthreads();
    s.dzd[lane] = dz_sum;
    __syncthreads();
    if (lane == 0) {
        double sum = 0.0;
        for (int q = 0; q < kPts; q++)
            sum += s.dzd[q];
        row[kBfOff] = sum;
    }
}

__global__ void cnn_points_reduce_kernel(const double *__restrict__ partial, int rows,
                                         float *__restrict__ grad_w)
{
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= kNP)
        return;
    double sum = 0.0;
    for (int g = 0; g < rows; g++)
        sum += partial[(size_t)g * kNP + j];
    grad_w[j] = (float)sum;
}

struct Plan {
    int passes, workgroups;
    size_t bytes;
};

int make_plan(const char *who, long long npoints, Plan *plan)
{
    if (npoints < 0)
        return fail(kBadArg, "%s: bad size P=%lld", who, npoints);
    if (npoints > 0x7fffffffll)
        return fail(kUnsupported, "%s: too many points for one launch", who);
    plan->passes = (int)((npoints + kPts - 1) / kPts);
    plan->workgroups = plan->passes < kMaxWgs ? plan->passes : kMaxWgs;
    plan->bytes = ((size_t)plan->workgroups * kNP * sizeof(double) + 15) & ~(size_t)15;
    return kOk;
}

}  // namespace
}  // namespace rft

extern "C" size_t rf_train_cnn_points_workspace_bytes(long long npoints)
{
    rft::Plan plan;
    if (rft::make_plan("rf_train_cnn_points_workspace_bytes", npoints, &plan) != rft::kOk)
        return 0;
    return plan.bytes;
}

extern "C" int rf_train_cnn_points_plan(long long npoints, int out[3])
{
    using namespace rft;
    if (!out)
        return fail(kBadArg, "rf_train_cnn_points_plan: NULL pointer");
    Plan plan;
    if (int bad = make_plan("rf_train_cnn_points_plan", npoints, &plan))
        return bad;
    out[0] = kPts;
    out[1] = plan.workgroups;
    out[2] = plan.workgroups;
    return kOk;
}

extern "C" int rf_train_cnn_points_backward_f32(const float *x, const float *weights,
                                                const float *grad_r, long long npoints,
                                                float *grad_w, void *workspace,
                                                size_t workspace_bytes, void *stream_)
{
    using namespace rft;
    const char *who = "rf_train_cnn_points_backward_f32";
    if (npoints == 0)  // no points: valid whatever the (possibly NULL) pointers are
        return kOk;
    Plan plan;
    if (int bad = make_plan(who, npoints, &plan))
        return bad;
    if (!x || !weights || !grad_r || !grad_w)
        return fail(kBadArg, "%s: NULL pointer", who);
    if (!workspace || workspace_bytes < plan.bytes || ((uintptr_t)workspace & 15))
        return fail(kBadArg, "%s: workspace of %zu bytes, %zu needed (16-byte aligned)", who,
                    workspace ? workspace_bytes : (size_t)0, plan.bytes);
    hipStream_t stream = (hipStream_t)stream_;
    double *partial = (double *)workspace;
    hipLaunchKernelGGL(cnn_points_backward_kernel, dim3((unsigned)plan.workgroups), dim3(kPts), 0,
                       stream, x, weights, grad_r, (int)npoints, plan.passes, partial);
    RFT_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(cnn_points_reduce_kernel, dim3((kNP + 255) / 256), dim3(256), 0, stream,
                       (const double *)partial, plan.workgroups, grad_w);
    RFT_HIP_CHECK(hipGetLastError());
    return kOk;
}
