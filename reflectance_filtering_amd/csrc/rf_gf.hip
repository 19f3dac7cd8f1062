// rf_gf.hip -- colour guided filter, uint8, for gfx950 (MI355X).
//
// Replaces cv2.ximgproc.guidedFilter(guide, src, radius, eps) as called at
// /root/reference/filter_reflectance.py:67-70.  Arithmetic contract (DESIGN.md "GF"): the
// operation order of opencv_contrib/modules/ximgproc/src/guided_filter.cpp (3-channel guide)
// over cv::boxFilter(CV_32F, normalize, BORDER_REFLECT) whose sums are double:
//
//   stage 1  box means of I_g, I_g*I_g', p_s, p_s*I_g.  Inputs are integers <= 65025, so the
//            double running sums OpenCV forms are exact integers; we form the same integers
//            with uint32 arithmetic (any order is exact) and round once:
//            mean = (float)((double)S * (1.0/k^2)).                         -> gf_stage1_kernel
//            The per-pixel algebra up to alpha/beta is fused behind it.
//   stage 2  box means of the float planes alpha_{s,g}, beta_s.  Not exact in double, so the
//            summation ORDER matters: RowSum<float,double> is a running sum along the
//            border-extended row starting at its left end, ColumnSum<double,float> a running
//            sum down the image starting 2r rows above the first output row.  Both are
//            reproduced as sequential chains (one lane per row / per column), exposed to the
//            GPU as parallelism over rows x planes x images, in two forms with identical bytes:
//            radius 1..128: gf_rowstate_kernel<R> + gf_colwalk_kernel<R> (rf_gf_fused.hpp,
//            instantiated per radius in rf_gf_fused_inst.hip) - the double row sums never reach
//            HBM; radius 0 (and the switch gf_two_kernel): gf_rowsum_kernel + gf_colsum_apply_kernel, which write
//            every row sum (8 B per pixel and plane) and read it twice; radius 129..4096: the
//            float kernels of rf_gf_f32 on float copies of the images, each pass rounded to uint8
//            (on 8-bit data their double window sums are the same exact integers).
//
// Grey sources: the reference filters the CNN's grey `-r.png`, which imread turns into three
// identical channels.  The src channels never mix, so identical channels give identical
// outputs; gf_grey_probe_kernel marks such images (a device-side flag, no host round trip) and
// they run the one-channel instantiation with the result byte written three times (1/3 of the
// per-channel planes).  Every stage is launched in both instantiations; workgroups of the one
// that does not apply to their image exit at once.  The probe also leaves channel 0 of every image
// as one byte per pixel in the workspace: that copy is what stage 1 reads for a grey image and
// what the passes of an iterated call hand on, until the last pass writes dst.
//
// Elsewhere:
//   rf_gf_stage1.hpp     stage 1: gf_stage1_kernel, its quantity structs, the grey probe and the plane
//                        interleave (this unit only).
//   rf_gf_algebra.hpp    Quant and the per-pixel algebra, shared by stage 1 and the float kernels.
//   rf_gf_twokernel.hpp  gf_rowsum_kernel / gf_colsum_apply_kernel (this unit: the 8-bit instantiations).
//   rf_gf_fused.hpp      the fused stage 2, instantiated per radius in rf_gf_fused_inst.hip.
//   rf_gf_f32.hip        the CV_32F filter (rf_gf_f32): its own kernels, the float instantiations of the pair.
//   rf_gf_common.hpp     the argument rules, the launch rule for a chunk, the side-stream functions.
//   rf_gf_side.hip       the side-stream table.
// Here, in order: the launch rule and the workspace arithmetic (gf_per_img_*, GfLayout, gf_layout,
// rf_gf_workspace_bytes); the uniform entry gf_u8_entry = argument rules -> gf_via_f32 (radius > 128) or
// gf_layout -> memset of the colour flags -> per chunk one part (gf_run_part) or the fork, two or more
// parts (gf_part_setup, gf_part_probe, then per pass gf_part_stage1, gf_part_stage2) and the join; the
// ragged planner (gf_ragged_check, gf_ragged_plan) and entry.
#include <algorithm>
#include <vector>

#include "rf_gf_common.hpp"
#include "rf_gf_stage1.hpp"
#include "rf_gf_twokernel.hpp"

namespace rf {

// The launch rule for a chunk of the uniform guided filter: the row and column walks fold the chunk's
// images into gridDim.x.  Does a chunk of m images of h x w fit every such launch (launch_fits)?
//   8-bit kernels: gf_rowstate_kernel m * src_cn * ceil(h / 64) workgroups of 256, gf_rowsum_kernel<4>
//   (two-kernel stage 2) four times as many of 64, gf_colwalk_kernel at most 8 * (ceil(m * nb / 8) + run) *
//   src_cn of 128 (its items per XCD rounded up to whole channel runs of 64, or of what the debug option
//   "gf_cw_chan_run" says), and under the debug option "gf_chained" the chained walk's 8 * ceil(m / 8) * src_cn *
//   nb of 128;
//   float kernels: gf_rowsum_kernel<1> m * (9 + 4 * src_cn) * ceil(h / 64) workgroups of 64.
bool gf_chunk_fits(int m, int h, int w, int src_cn, bool float_kernels)
{
    // (64-bit: h may be anything up to INT_MAX here, where ceil_div's h + 63 would overflow an int)
    const unsigned long long mm = (unsigned long long)m, rb = ((unsigned long long)h + kBRows - 1) / kBRows;
    if (float_kernels)
        return launch_fits(mm * (9 + 4 * src_cn) * rb, 64);
    const unsigned long long nb = ((unsigned long long)w + kSB - 1) / kSB;
    const unsigned long long run = (unsigned long long)std::max(64, debug_get(kDbgGfCwChanRun));
    return launch_fits(mm * src_cn * rb, 256) && launch_fits(mm * 4 * src_cn * rb, 64) &&
           launch_fits(8 * ((mm * nb + 7) / 8 + run) * src_cn, 128) &&
           (!debug_get(kDbgGfChained) || launch_fits(8 * ((mm + 7) / 8) * src_cn * nb, 128));
}

// The largest chunk of at most `chunk` images that fits (0: not even one image does).
int gf_launch_chunk(int chunk, int h, int w, int src_cn, bool float_kernels)
{
    int lo = 0, hi = chunk;  // lo fits (or is 0), everything above hi does not
    while (lo < hi) {
        const int mid = lo + (hi - lo + 1) / 2;
        if (gf_chunk_fits(mid, h, w, src_cn, float_kernels))
            lo = mid;
        else
            hi = mid - 1;
    }
    return lo;
}

namespace {
// uint8 <-> float images for radii beyond the 8-bit kernels' range (rf_gf_u8 -> float kernels)
__global__ __launch_bounds__(256) void gf_u8_to_f32_kernel(const uint8_t *__restrict__ in,
                                                           float *__restrict__ out, size_t count)
{
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < count;
         i += (size_t)gridDim.x * blockDim.x)
        out[i] = (float)in[i];
}
// ... and a grey guide (one byte per pixel) into the three equal float channels the float kernels take
__global__ __launch_bounds__(256) void gf_u8_grey_to_f32x3_kernel(const uint8_t *__restrict__ in,
                                                                  float *__restrict__ out, size_t count)
{
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < count;
         i += (size_t)gridDim.x * blockDim.x) {
        const float v = (float)in[i];
        out[3 * i + 0] = v;
        out[3 * i + 1] = v;
        out[3 * i + 2] = v;
    }
}
__global__ __launch_bounds__(256) void gf_f32_to_u8_kernel(const float *__restrict__ in,
                                                           uint8_t *__restrict__ out, size_t count)
{
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < count;
         i += (size_t)gridDim.x * blockDim.x)
        out[i] = saturate_u8(in[i]);  // convertTo(CV_8U): round half to even, clamp, NaN -> 0
}

}  // namespace

// The per-radius launchers live in the rf_gf_fused_<part>.o units (Makefile: GF_PARTS = 8).
GfFusedLaunch gf_fused_part_0(int), gf_fused_part_1(int), gf_fused_part_2(int), gf_fused_part_3(int),
    gf_fused_part_4(int), gf_fused_part_5(int), gf_fused_part_6(int), gf_fused_part_7(int);
// ... and the radii above kGfFusedSmallMax in rf_gf_fused_L<part>.o (GF_LARGE_PARTS = 4)
GfFusedLaunch gf_fused_large_0(int), gf_fused_large_1(int), gf_fused_large_2(int), gf_fused_large_3(int);

GfFusedLaunch gf_fused_launcher(int radius)
{
    typedef GfFusedLaunch (*Part)(int);
    static const Part parts[8] = {gf_fused_part_0, gf_fused_part_1, gf_fused_part_2, gf_fused_part_3,
                                  gf_fused_part_4, gf_fused_part_5, gf_fused_part_6, gf_fused_part_7};
    if (radius < 1 || radius > kGfFusedMaxRadius)
        return nullptr;
    if (radius > kGfFusedSmallMax) {
        static const Part large[4] = {gf_fused_large_0, gf_fused_large_1, gf_fused_large_2, gf_fused_large_3};
        return large[(radius - kGfFusedSmallMax - 1) % 4](radius);
    }
    return parts[(radius - 1) % 8](radius);
}

size_t gf_workspace_cap()
{
    static size_t cap = 0;  // the answer cannot change within a process; a benign race at worst
    if (cap == 0) {
        size_t c = (size_t)6 << 30;
        int dev = 0;
        hipDeviceProp_t prop;
        if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess)
            c = std::min(std::max(c, (size_t)prop.totalGlobalMem / 8), (size_t)32 << 30);
        else
            (void)hipGetLastError();  // no device: not an error of this call
        cap = c;
    }
    return cap;
}

// per-image "has colour" flags at the head of the workspace
size_t gf_header_bytes(int n) { return (((size_t)n * sizeof(int)) + 255) & ~(size_t)255; }

}  // namespace rf

namespace rf {
// Scratch per image in flight, by stage-2 form (np = 4 x src channels float planes alpha/beta):
//   two-kernel   alpha/beta + a double row sum per pixel and plane
//   row walk     alpha/beta + a double state per 16 pixels and plane
//   chained      alpha/beta + the hand-off words (16 B per lane, 64 lanes per sub-tile and block)
//                + the head sums (a double per row and plane) + the part's sync words
size_t gf_per_img_two_kernel(size_t npx, int np) { return npx * np * (sizeof(float) + sizeof(double)); }
size_t gf_per_img_row_walk(size_t npx, int np, int nb, int h)
{
    return (size_t)np * (npx * sizeof(float) + (size_t)nb * h * sizeof(double));
}
// exact rows: per image and plane group the statistics of stage 1 (8 B per half-wave and row; a strip
// has at least 256 output columns for every radius the 8-bit kernels take), a flag byte and a list
// entry per row, the list's length
size_t gf_exact_extra(int np, int h, int w)
{
    const size_t slots = (size_t)ceil_div(w, 256) * 8;
    return (((size_t)(np / 4) * ((size_t)h * (slots * 8 + 8) + 16)) + 255) & ~(size_t)255;
}
// 3-channel sources handed from pass to pass in the workspace (gf_layout): one byte per pixel of a grey
// image, three planes of a colour image; rounded up so that the parts stay 16-byte aligned
size_t gf_compact_bytes(size_t npx) { return (npx + 15) & ~(size_t)15; }
size_t gf_compact3_bytes(size_t npx) { return (3 * npx + 15) & ~(size_t)15; }
constexpr size_t kGfSyncBytes = 256;
// radii above this run the float kernels (uint32 window sums: (2r+1)^2 * 255^2 < 2^32)
constexpr int kGfMaxRadiusU8 = 128;  // (2 * 128 + 1)^2 * 255^2 = 4,294,836,225 < 2^32: the last radius that fits
// ... on float copies of guide, src and result + the float kernels' own planes and row sums
constexpr size_t kGfF32Slack = 16;  // once per workspace: alignment of the float kernels' scratch
size_t gf_per_img_via_f32(size_t npx, int src_cn)
{
    return npx * ((3 + 2 * (size_t)src_cn) * sizeof(float) +
                  (9 + 4 * (size_t)src_cn) * (sizeof(float) + sizeof(double)));
}
size_t gf_chain_xst_bytes(int src_cn, int nb, int h, int radius)
{
    return (size_t)src_cn * nb * gf_chain_nsub(h, radius) * 64 * 16;
}
size_t gf_per_img_chained(size_t npx, int np, int nb, int h, int radius)
{
    return kGfSyncBytes + gf_chain_xst_bytes(np / 4, nb, h, radius) + (size_t)np * h * sizeof(double) +
           npx * np * sizeof(float);
}
}  // namespace rf

#ifdef RF_GF_S1_STAMP
extern "C" int rf_debug_gf_s1_stamps(unsigned long long *out16)
{
    unsigned long long zero[16] = {};
    if (hipMemcpyFromSymbol(out16, HIP_SYMBOL(rf::g_s1_stamps), sizeof(zero)) != hipSuccess)
        return -4;
    if (hipMemcpyToSymbol(HIP_SYMBOL(rf::g_s1_stamps), zero, sizeof(zero)) != hipSuccess)
        return -4;
    return 0;
}
#endif

extern "C" size_t rf_gf_workspace_bytes(int n, int h, int w, int guide_cn, int src_cn, int radius)
{
    (void)guide_cn;
    if (n <= 0 || h <= 0 || w <= 0 || (src_cn != 1 && src_cn != 3))
        return 0;
    // the larger of the forms a call may take (small images: the chained form's fixed part)
    size_t per_img = rf::gf_per_img_two_kernel((size_t)h * w, 4 * src_cn);
    if (radius > rf::kGfMaxRadiusU8)  // float kernels on float copies of the images (rf_gf_u8)
        per_img = rf::gf_per_img_via_f32((size_t)h * w, src_cn);
    if (radius >= 1 && radius <= rf::kGfFusedMaxRadius) {
        per_img = std::max(per_img, rf::gf_per_img_chained((size_t)h * w, 4 * src_cn,
                                                           rf::ceil_div(w, rf::kSB), h, radius));
        per_img = std::max(per_img, rf::gf_per_img_row_walk((size_t)h * w, 4 * src_cn,
                                                            rf::ceil_div(w, rf::kSB), h) +
                                        rf::gf_exact_extra(4 * src_cn, h, w) +
                                        rf::gf_compact_bytes((size_t)h * w) +
                                        (src_cn == 3 ? rf::gf_compact3_bytes((size_t)h * w) : 0));
    }
    // enough images in flight to fill the chip and to make the tails of the launches small: capped
    // at 1/8 of the device's memory, at most 32 GiB (6 GiB when no device can be asked).  C5 shard
    // (128 x 4K, 3 passes): round 2 91.5 ms with 6 GiB (13 images per chunk), 86.6 ms with 16 GiB (37);
    // round 3 70.7 / 68.6 / 70.1 ms with 16 / 32 / 64 GiB (chunks of 37 / 74 / all 128 images).
    size_t imgs = (size_t)n;
    const size_t cap = rf::gf_workspace_cap();
    if (imgs * per_img > cap)
        imgs = cap / per_img;
    if (imgs < 1)
        imgs = 1;
    return rf::gf_header_bytes(n) + imgs * per_img + (radius > rf::kGfMaxRadiusU8 ? rf::kGfF32Slack : 0);
}

namespace {
using namespace rf;
// stage-1 strips of a w-column image (see the comment in gf_layout): the left halo, the output
// columns of a strip and how many strips cover the row.  hl and out_w depend on the radius, the
// channel count and the guide kind - and on w only through the choice of the whole-wave halo, which is
// taken where it costs no strip.
struct StripGeom {
    int hl, out_w, strips;
};
StripGeom gf_strip_geometry(int radius, int w, int scn, bool grey)
{
    const int acw = stage1_threads(scn, grey) * stage1_cols(scn, grey);
    StripGeom g;
    if (debug_get(kDbgGfS1LegacyStrips)) {
        g.hl = radius;
        g.out_w = acw - 2 * radius;
    } else {
        g.hl = (radius + 15) & ~15;
        g.out_w = (acw - g.hl - radius) & ~15;
        if (radius <= 64 && ceil_div(w, acw - 128) <= ceil_div(w, g.out_w)) {
            g.hl = 64;
            g.out_w = acw - 128;
        }
    }
    g.strips = ceil_div(w, g.out_w);
    return g;
}

// Rows per stage-1 segment of an h-row image whose rows of segments hold strips_k strips (the rule
// and its measurements: the comment in gf_part_setup).  m_fill = images whose stage 1 is in
// flight together, m_part = images of this launch.
int gf_pick_seg(int h, int radius, int strips_k, int m_fill, int m_part, long long min_wgs, int cap,
                int per_cu)
{
    int seg;
    if (debug_get(kDbgGfS1MinWgs) > 0) {  // the round-4 rule, kept for A/B runs
        min_wgs = debug_get(kDbgGfS1MinWgs);
        const long long per_seg = std::max<long long>(1, (long long)strips_k * m_fill);
        long long k = (min_wgs + per_seg - 1) / per_seg;          // segments per image
        k = std::max<long long>(k, ceil_div(h, cap));
        k = std::min<long long>(std::max<long long>(k, 1), h);
        seg = ceil_div(h, (int)k);
        seg = std::max(seg, std::min(h, std::max(3 * (2 * radius + 1) / 4, 32)));
    } else {
        const double warm = 0.2 * 2.0 * radius;
        // time of k resident workgroups on one CU, in units of one workgroup alone
        static const double crowd[5] = {0.0, 1.0, 2.0 / 1.38, 3.0 / 1.70, 4.0 / 1.87};
        const long long slots = 256LL * per_cu;
        double best = 0.0;
        seg = h;
        // (k runs over the segment counts that change the segment length: O(sqrt(h)) of them)
        for (int k = std::max(1, ceil_div(h, cap)); k <= h;) {
            const int sg = ceil_div(h, k);
            const int k_next = sg > 1 ? (h - 1) / (sg - 1) + 1 : h + 1;
            // full rounds of resident workgroups, then the rest on ceil(rest / 256) per CU: a
            // launch a little over a whole round pays a whole workgroup's length for the rest
            // (4 colour images at 4K: 800 workgroups on 768 places 2.47 ms, 640 on them 2.26)
            // (two halves on two streams: the other half's kernels fill the tail of a launch,
            //  so beyond one round the workgroups are priced as a fluid - at the C5 shard that
            //  keeps round 4's three segments of 720 rows, 63.4 against 64.4 ms with 540)
            const long long wgs = (long long)strips_k * m_fill * ceil_div(h, sg);
            const long long full = wgs / slots, rest = wgs % slots;
            const double t =
                (m_fill > m_part && wgs > slots)
                    ? (warm + sg) * (double)wgs / (double)slots * crowd[per_cu]
                    : (warm + sg) * ((double)full * crowd[per_cu] +
                                     (rest ? crowd[(int)((rest + 255) / 256)] : 0.0));
            if (best == 0.0 || t < best * 0.999) {
                best = t;
                seg = sg;
            }
            k = std::max(k + 1, k_next);
        }
    }
    seg = ceil_div(h, ceil_div(h, seg));  // equal segments: a launch ends with its longest one
    if (debug_get(kDbgGfSegRows) > 0)
        seg = std::min(h, debug_get(kDbgGfSegRows));
    return seg;
}

// ------------------------------------------------------------------------------------------
// The uniform entry (rf_gf_u8, rf_gf_ex_u8; `fn`: the entry point named in error messages) in parts:
// gf_via_f32, the layout decision (GfLayout, gf_layout), the call context (GfCall), a part and its steps
// (Part, gf_part_*), the staggered schedule, gf_u8_entry.
// ------------------------------------------------------------------------------------------

// Beyond the 8-bit kernels' range (int(sigma_spatial) is a free parameter of the reference's
// tool, /root/reference/filter_reflectance.py:67-70,118): the float kernels of rf_gf_f32 on
// float copies of the images, every pass rounded to uint8 like convertTo(CV_8U).  On 8-bit
// data the float path's double window sums are the same exact integers the 8-bit stage 1
// forms, so the bytes are what the 8-bit kernels would give (tested on either side of 128).
int gf_via_f32(const char *fn, const uint8_t *guide, const uint8_t *src, uint8_t *dst, int n, int h, int w,
               int src_cn, int radius, double eps, int iterations, bool grey, void *workspace,
               size_t workspace_bytes, void *stream_)
{
    const size_t npx = (size_t)h * w;
    const size_t header = gf_header_bytes(n);
    const int gcn = grey ? 1 : 3;  // guide bytes per pixel
    hipStream_t stream = (hipStream_t)stream_;
    const size_t per_img_f = gf_per_img_via_f32(npx, src_cn);
    if (workspace_bytes < header + per_img_f + kGfF32Slack)
        return fail(RF_E_WORKSPACE, "%s: workspace %zu B < %zu B needed for one image at "
                    "radius %d", fn, workspace_bytes, header + per_img_f + kGfF32Slack, radius);
    const size_t f32_ws = npx * (9 + 4 * (size_t)src_cn) * (sizeof(float) + sizeof(double));
    // (kGfF32Slack: the float kernels' scratch starts with double row sums, so the float copies
    //  in front of it are rounded up to 16 bytes - an odd pixel count would leave it 4-aligned)
    int chunk = (int)std::min<size_t>((size_t)n, (workspace_bytes - header - kGfF32Slack) / per_img_f);
    // gf_f32_chunk puts the image index in gridDim.y / .z and folds the chunk into gridDim.x
    chunk = gf_launch_chunk(std::min(chunk, kMaxGridYZ), h, w, src_cn, true);
    if (chunk == 0)
        return fail(RF_E_UNSUPPORTED, "%s: an image of %d x %d is too large for one launch", fn, w, h);
    char *ws0 = static_cast<char *>(workspace) + header;
    for (int i0 = 0; i0 < n; i0 += chunk) {
        const int m = std::min(chunk, n - i0);
        float *gF = reinterpret_cast<float *>(ws0);
        float *sF = gF + (size_t)m * npx * 3;
        float *dF = sF + (size_t)m * npx * src_cn;
        const size_t copies = ((size_t)m * npx * (3 + 2 * (size_t)src_cn) * sizeof(float) + 15) & ~(size_t)15;
        void *fw = ws0 + copies;
        const size_t cg = (size_t)m * npx * gcn, cs = (size_t)m * npx * src_cn;
        const unsigned bg = (unsigned)std::min<size_t>((cg + 255) / 256, 65535);
        const unsigned bs = (unsigned)std::min<size_t>((cs + 255) / 256, 65535);
        if (grey)  // expanded to the three equal channels while copying
            hipLaunchKernelGGL(gf_u8_grey_to_f32x3_kernel, dim3(bg), dim3(256), 0, stream,
                               guide + (size_t)i0 * npx, gF, cg);
        else
            hipLaunchKernelGGL(gf_u8_to_f32_kernel, dim3(bg), dim3(256), 0, stream,
                               guide + (size_t)i0 * npx * 3, gF, cg);
        uint8_t *d0 = dst + (size_t)i0 * npx * src_cn;
        for (int it = 0; it < iterations; it++) {
            const uint8_t *s0 = it == 0 ? src + (size_t)i0 * npx * src_cn : d0;
            hipLaunchKernelGGL(gf_u8_to_f32_kernel, dim3(bs), dim3(256), 0, stream, s0, sF, cs);
            const int rc = rf_gf_f32(gF, sF, dF, m, h, w, 3, src_cn, radius, eps, 1, fw,
                                     (size_t)m * f32_ws, stream_);
            if (rc != RF_OK)
                return rc;
            hipLaunchKernelGGL(gf_f32_to_u8_kernel, dim3(bs), dim3(256), 0, stream, dF, d0, cs);
        }
    }
    RF_HIP_CHECK(hipGetLastError());
    return RF_OK;
}

// What a call at radius 0..kGfMaxRadiusU8 keeps per image in its workspace, which form its stage 2
// takes and how its stage 1 is cut into strips: decided once per call by gf_layout from the sizes, the
// radius, the debug options and the workspace the caller gave.
struct GfLayout {
    GfFusedLaunch fused_launch;  // the radius's fused stage 2 (nullptr: not instantiated)
    bool fused, chained;         // stage 2: fused (row walk + column walk, or the chained column walk) | the kernel pair
    bool keep_gs;                // "gf_guide_cache": the guide half of the algebra kept for later passes
    bool exact;                  // "gf_exact": exact rows
    size_t gs_bytes;             // per image: the guide record (where keep_gs)
    size_t cmp_bytes, cmp3_bytes;  // per image: the one-byte and the three-plane hand-off (0: none)
    size_t exact_bytes;          // per image: the exact rows' statistics (where exact)
    size_t per_img_used;         // per image, everything
    int chunk;                   // images in flight together
    GfStateLayout lay;           // where a (plane, block, row) state / block sum sits
    StripGeom geo1, geo3;        // stage-1 strips of the one- and the three-channel kernel
    int xslots, mask_words;      // exact rows: statistic slots per row, words of a row bitmask
    unsigned pad1, pad3;         // stage 1: dynamic-LDS pad of the occupancy cap ("gf_s1_cap")
};

int gf_layout(const char *fn, int n, int h, int w, int src_cn, int radius, int iterations, bool grey,
              size_t workspace_bytes, GfLayout *out)
{
    GfLayout &L = *out;
    const int np = 4 * src_cn;
    const size_t npx = (size_t)h * w;
    const int nb = ceil_div(w, kSB);
    const size_t header = gf_header_bytes(n);
    // Stage 2 (box means of alpha/beta), three forms with identical bytes:
    //   row walk + column walk (default for the instantiated radii 1..96)
    //   chained column walk (debug option "gf_chained", radius 45 and 52 only: no row-walk kernel, every block takes its row
    //       sums from its left neighbour; identical bytes, measured SLOWER - the stagger between
    //       neighbouring blocks costs the L2 sharing of their operand lines, profiles/r04_gf_chained.md)
    //   row-sum / column-sum kernel pair (radius 0; debug option "gf_two_kernel")
    // (the fused kernels index planes with 32-bit element offsets: images below 2^28 pixels)
    L.fused_launch = gf_fused_launcher(radius);
    const bool can_fuse = !debug_get(kDbgGfTwoKernel) && L.fused_launch != nullptr &&
                          npx < ((size_t)1 << 28);
    const size_t per_img_chained = can_fuse ? gf_per_img_chained(npx, np, nb, h, radius) : 0;
    const size_t per_img_rw = gf_per_img_row_walk(npx, np, nb, h);
    const size_t per_img = gf_per_img_two_kernel(npx, np);
    L.chained = can_fuse && debug_get(kDbgGfChained) && gf_chained_radius(radius) &&
                workspace_bytes >= header + per_img_chained;
    L.fused = L.chained || (can_fuse && workspace_bytes >= header + per_img_rw);
    const size_t per_img_fused = L.chained ? per_img_chained : per_img_rw;
    if (!L.fused && workspace_bytes < header + per_img)
        return fail(RF_E_WORKSPACE, "%s: workspace %zu B < %zu B needed for one image", fn,
                    workspace_bytes, header + per_img);
    // EXPERIMENT, off by default (debug option "gf_guide_cache"): iterated calls keep the guide half
    // of the per-pixel algebra (kGsFloats floats per pixel) from the first pass for the later ones,
    // which then box-sum only the 4 src quantities - 3x fewer VALU instructions in stage 1, but 36
    // more bytes per pixel and pass through a memory system the other kernels of the pass already
    // load.  Measured twice (interleaved 36-byte records; row-planar records with coalesced
    // accesses), 8 x 4K grey, kernels alone: stage 1 of a later pass 1.085 ms against 1.044 ms
    // without the record, the pass that writes it 1.69 ms; C5 shard 11.4 against 14.0 GP/s
    // (profiles/r03_gf_guide_cache.md).  Kept as a switch so that the measurement can be repeated.
    L.gs_bytes = (npx * kGsFloats * sizeof(float) + 15) & ~(size_t)15;  // parts stay 16-byte aligned
    L.keep_gs = iterations > 1 && debug_get(kDbgGfGuideCache) &&
                workspace_bytes - header >= (L.fused ? per_img_fused : per_img) + L.gs_bytes;
    // 3-channel sources: an image whose channels are equal (the reference filters the CNN's grey map,
    // /root/reference/README.md:66) is handled as ONE byte per pixel in the workspace: the grey
    // probe, which reads every src byte anyway, leaves channel 0 there for the first pass's stage 1
    // (its one-byte-per-pixel instantiation fetches 4 instead of 6 bytes per pixel and row), and the
    // passes of an iterated call hand their result on the same way - the column walk writes a third
    // of the bytes - until the last pass writes dst.  Bytes identical (debug option "gf_no_compact"
    // keeps the three-channel reads and hand-offs).
    const size_t cmp_want = gf_compact_bytes(npx);
    L.cmp_bytes = (L.fused && src_cn == 3 && !debug_get(kDbgGfNoCompact) &&
                   workspace_bytes - header >= per_img_fused + (L.keep_gs ? L.gs_bytes : 0) + cmp_want)
                      ? cmp_want
                      : 0;
    // Colour images leave every pass as three PLANES in the workspace (round 6): a channel's column
    // walk then stores 4 bytes per lane instead of four single bytes into the interleaved dst (its
    // vector-memory instructions are what it is short of), stage 1 of the next pass reads bytes either
    // way, and a small kernel interleaves the last pass's planes into dst (6 B/px at copy speed).
    const size_t cmp3_want = gf_compact3_bytes(npx);
    L.cmp3_bytes = (L.cmp_bytes && !L.keep_gs &&
                    workspace_bytes - header >= per_img_fused + L.cmp_bytes + cmp3_want)
                       ? cmp3_want
                       : 0;
    // Exact rows (rf_gf_fused.hpp): rows whose alpha/beta pass the exactness test need no row walk -
    // stage 1 leaves block sums and per-row statistics, the rows that fail are listed and walked, the
    // column walk starts its chains from the block sums.  Needs a width that is a multiple of 16 and
    // room for the statistics.  OFF unless the debug option "gf_exact" is set: bit-identical, measured
    // slower than the row walk (profiles/r06_gf_exact.md); compiled for the radii of gf_exact_radius.
    L.exact_bytes = gf_exact_extra(np, h, w);
    L.exact = L.fused && !L.chained && !L.keep_gs && gf_exact_radius(radius) && w % 16 == 0 &&
              h <= kGfExactMaxH && debug_get(kDbgGfExact) && !debug_get(kDbgGfS1LegacyStrips) &&
              workspace_bytes - header >= per_img_fused + L.cmp_bytes + L.cmp3_bytes + L.exact_bytes;
    L.per_img_used = (L.fused ? per_img_fused : per_img) + (L.keep_gs ? L.gs_bytes : 0) + L.cmp_bytes +
                     L.cmp3_bytes + (L.exact ? L.exact_bytes : 0);
    L.chunk = (int)std::min<size_t>((size_t)n, (workspace_bytes - header) / L.per_img_used);
    // at most 16383 images (gridDim.y holds image x channel), and no more than the row and column walks'
    // launches take, which fold the chunk into gridDim.x
    L.chunk = gf_launch_chunk(std::min(L.chunk, 16383), h, w, src_cn, false);
    if (L.chunk == 0)
        return fail(RF_E_UNSUPPORTED, "%s: an image of %d x %d is too large for one launch", fn, w, h);
    // chained column walk: a part's images are dealt to 8 ticket queues (one per XCD), so parts of
    // a multiple of 8 images - chunks of a multiple of 16 - load the queues evenly
    if (L.chained && L.chunk >= 16 && n > L.chunk)
        L.chunk &= ~15;
    // stage-1 strips: stage1_threads x stage1_cols columns, at least r of them halo on either side.
    // The left halo and the output width are multiples of 16 (a 16-lane row of the per-pixel phase
    // is then one aligned 16-column block of the image); a halo of a whole wave on either side is
    // taken where it costs no strip (two of the strip's wave-iterations then have nothing to do, see
    // the kernel).  Debug option "gf_s1_legacy_strips": halo r on either side (rounds 1-5).
    L.geo3 = gf_strip_geometry(radius, w, 3, grey);
    L.geo1 = gf_strip_geometry(radius, w, 1, grey);
    L.xslots = std::max(L.geo1.strips, L.geo3.strips) * 8;  // exact rows: statistic slots per row
    L.mask_words = ceil_div(h, 32);
    L.lay = L.exact ? GfStateLayout{nb, 1, 4 * nb} : GfStateLayout{nb * h, h, 1};
    // stage-1 occupancy cap (debug option "gf_s1_cap" = workgroups per CU, 0 = whatever fits): a
    // dynamic-LDS pad makes one more workgroup than the cap exceed the CU's 160 KB, which leaves
    // registers and LDS on every CU for the walk kernels of the other part (see the schedules)
    const int s1_cap = debug_get(kDbgGfS1Cap);
    auto s1_pad = [&](int scn) -> unsigned {
        const int nq = stage1_nq(scn, grey);
        const size_t static_lds =
            sizeof(uint32_t) * (nq * (stage1_threads(scn, grey) * stage1_cols(scn, grey) + 1) + nq * 4);
        if (s1_cap < 1 || s1_cap > 3)
            return 0;
        const size_t want = (size_t)163840 / (s1_cap + 1) + 1536;
        return want > static_lds ? (unsigned)(want - static_lds) : 0u;
    };
    L.pad1 = s1_pad(1);
    L.pad3 = s1_pad(3);
    return RF_OK;
}

// What the steps of a call's parts read: the caller's arguments, what follows from them, the layout.
struct GfCall {
    const uint8_t *guide, *src;
    uint8_t *dst;
    int h, w, src_cn, radius, iterations;
    bool grey;
    int gcn;          // guide bytes per pixel
    int np, nb;       // alpha/beta planes per image; 16-column blocks per row
    size_t npx;       // pixels per image
    float eps_f;
    int eps_small;
    int *colour_all;  // 3-channel sources: the per-image "has colour" flags (head of the workspace)
    int probe_blocks;
    GfLayout L;
};

// One part = m images starting at i0, their scratch at ws, every launch on st.  A part is
// enqueued in steps - probe, then per pass stage 1 and stage 2 - so that the schedules can
// interleave the steps of several parts.
struct Part {
    int i0, m;
    char *ws;
    hipStream_t st;
    // derived (gf_part_setup)
    const int *colour;
    double *rows;
    float *ab, *gs;
    uint8_t *cmp, *cmp3;
    uint2 *xstat;            // exact rows: statistics, list and its lengths, flag bitmask
    unsigned *rowmask;
    int *xlist, *xcount;
    GfChain xc;
    const uint8_t *g0;
    uint8_t *d0;
    int seg_rows1, seg_rows3;
};

void gf_part_setup(const GfCall &c, Part &P, int m_fill)
{
    const GfLayout &L = c.L;
    const int i0 = P.i0, m = P.m, h = c.h, np = c.np, nb = c.nb;
    const size_t npx = c.npx;
    char *ws = P.ws;
    P.colour = c.colour_all ? c.colour_all + i0 : nullptr;
    // two-kernel form: [row sums (double)][alpha/beta]; row walk: [states (double)][alpha/beta];
    // chained: [sync words][hand-off words][head sums][alpha/beta]
    P.rows = reinterpret_cast<double *>(ws);
    P.ab = reinterpret_cast<float *>(P.rows + (L.fused ? (size_t)m * np * nb * h
                                                        : (size_t)m * np * npx));
    P.xc = GfChain{nullptr, nullptr, nullptr};
    if (L.chained) {
        P.xc.sync = reinterpret_cast<unsigned *>(ws);
        P.xc.xst = reinterpret_cast<unsigned long long *>(ws + kGfSyncBytes);
        double *head = reinterpret_cast<double *>(
            ws + kGfSyncBytes + (size_t)m * gf_chain_xst_bytes(c.src_cn, nb, h, c.radius));
        P.xc.head = head;
        P.ab = reinterpret_cast<float *>(head + (size_t)m * np * h);
        P.rows = nullptr;
    }
    P.gs = L.keep_gs ? P.ab + (size_t)m * np * npx : nullptr;  // [m][h][kGsFloats][w]
    // grey 3-channel images of an iterated call: the passes hand their result on as one byte per
    // pixel (see cmp_bytes in gf_layout)
    P.cmp = L.cmp_bytes ? reinterpret_cast<uint8_t *>(P.ab + (size_t)m * np * npx) +
                              (L.keep_gs ? (size_t)m * L.gs_bytes : 0)
                        : nullptr;
    P.cmp3 = L.cmp3_bytes ? P.cmp + (size_t)m * L.cmp_bytes : nullptr;  // [m][3][npx]
    P.xstat = nullptr;
    P.rowmask = nullptr;
    P.xlist = P.xcount = nullptr;
    if (L.exact) {
        char *xb = reinterpret_cast<char *>(P.ab + (size_t)m * np * npx) +
                   (L.keep_gs ? (size_t)m * L.gs_bytes : 0) + (size_t)m * (L.cmp_bytes + L.cmp3_bytes);
        const size_t rows_all = (size_t)m * c.src_cn * h;
        P.xstat = reinterpret_cast<uint2 *>(xb);
        P.xlist = reinterpret_cast<int *>(P.xstat + rows_all * L.xslots);
        P.xcount = P.xlist + rows_all;  // [m x groups] lengths, then [m x groups][mask_words] flags
        P.rowmask = reinterpret_cast<unsigned *>(P.xcount + (size_t)m * c.src_cn);
    }
    P.g0 = c.guide + (size_t)i0 * npx * c.gcn;
    P.d0 = c.dst + (size_t)i0 * npx * c.src_cn;
    // Rows per stage-1 segment (m_fill: the images whose stage 1 is in flight on the device
    // together - both halves of a chunk in the aligned schedule, the part alone otherwise).  A
    // workgroup walks its 2r warm-up rows (about a fifth of a main row each: sums only) and then its
    // segment; more, shorter segments spread small work over the chip, fewer and longer ones waste
    // less on warm-up rows and re-read fewer bytes.  A small cost model decides: k workgroups
    // resident on a CU take crowd[k] times one workgroup alone (one wave per SIMD issues every ~6
    // cycles, four saturate the pipe - stage 1 alone at 1 / 2 / 3 / 4 workgroups per CU,
    // profiles/r05_c5_overlap.md: k / 1, 1.38, 1.70, 1.87); a launch is whole rounds of resident
    // workgroups plus the rest; the segment count with the least modelled time wins.  Against the
    // round-4 rule (>= 960 workgroups, never below 3/4 of a window: debug option "gf_s1_min_wgs" =
    // 960), ms per call: 1 x 256x256 0.10 / 0.28, 1 x IIW 0.11 / 0.31, 1 x 1080p 0.26 / 0.44,
    // 1 x 4K 0.48 / 0.58, 2 x 4K 0.67 / 0.74, 16 x IIW 0.25 / 0.42, 4 x 4K colour 2.12 / 2.24,
    // 32 x 4K x 3 passes 16.6 / 17.5, 64 x 1080p x 3 8.7 / 9.2; equal at 4 x 4K, 256 x IIW and the
    // C5 shard, which keeps the three segments of 720 rows measured best in round 4
    // (profiles/r05_gf_seg_sweep.json; the measurements behind the earlier rules: HISTORY.md).
    // The 3-channel kernel (21 running sums, 3 workgroups per CU) is capped at 6 windows per segment.
    P.seg_rows1 = gf_pick_seg(h, c.radius, L.geo1.strips, m_fill, m, 960, h, 4);
    P.seg_rows3 = gf_pick_seg(h, c.radius, L.geo3.strips, m_fill, m, 1024,
                              std::max(6 * (2 * c.radius + 1), 512), 3);
}

// the part's grey probe (flags zeroed by the caller's stream before the fork); with the
// one-byte hand-off it also leaves every image's channel 0 in cmp for the first pass
void gf_part_probe(const GfCall &c, const Part &P)
{
    if (c.colour_all != nullptr)
        hipLaunchKernelGGL(gf_grey_probe_kernel, dim3(c.probe_blocks, P.m), dim3(256), 0, P.st,
                           c.src + (size_t)P.i0 * c.npx * 3, c.colour_all + P.i0, c.npx, P.cmp);
}

// (the occupancy cap's dynamic-LDS pad can take a workgroup beyond the 64 KB a launch may use
//  without asking: ask)
template <class K>
void gf_s1_attr(K kernel, unsigned pad)
{
    if (pad > 0)
        (void)hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)pad);
}

// Stage 1 of pass `it` of a part in one of its forms: both instantiations for a 3-channel source (the
// one-channel one reads the one-byte copy where the part has it), the one-channel one otherwise.
template <int MODE, bool EXACT, bool GREY>
void launch_stage1(const GfCall &c, const Part &P, int it)
{
    const GfLayout &L = c.L;
    hipStream_t st = P.st;
    const int h = c.h, w = c.w, radius = c.radius;
    const uint8_t *s0 = (it == 0 ? c.src : (const uint8_t *)c.dst) + (size_t)P.i0 * c.npx * c.src_cn;
    const dim3 ga3(L.geo3.strips, ceil_div(h, P.seg_rows3), P.m), ga1(L.geo1.strips, ceil_div(h, P.seg_rows1), P.m);
    const dim3 threads3(stage1_threads(3, GREY)), threads1(stage1_threads(1, GREY));
    const GfExactOut xo = {P.rows, P.xstat, c.nb, L.xslots};
    const GfRagged no_rag = {nullptr, nullptr};
    gf_s1_attr(gf_stage1_kernel<3, 3, MODE, EXACT, GREY>, L.pad3);
    gf_s1_attr(gf_stage1_kernel<1, 1, MODE, EXACT, GREY>, L.pad1);
    gf_s1_attr(gf_stage1_kernel<1, 3, MODE, EXACT, GREY>, L.pad1);
    if (c.src_cn == 3) {
        hipLaunchKernelGGL((gf_stage1_kernel<3, 3, MODE, EXACT, GREY>), ga3, threads3, L.pad3, st, P.g0, s0,
                           P.ab, h, w, radius, c.eps_f, c.eps_small, P.seg_rows3, P.colour, P.gs, 3,
                           L.geo3.hl, L.geo3.out_w, xo, it > 0 ? P.cmp3 : nullptr, no_rag);
        if (P.cmp != nullptr)
            hipLaunchKernelGGL((gf_stage1_kernel<1, 1, MODE, EXACT, GREY>), ga1, threads1, L.pad1, st, P.g0,
                               P.cmp, P.ab, h, w, radius, c.eps_f, c.eps_small, P.seg_rows1, P.colour,
                               P.gs, 3, L.geo1.hl, L.geo1.out_w, xo, nullptr, no_rag);
        else
            hipLaunchKernelGGL((gf_stage1_kernel<1, 3, MODE, EXACT, GREY>), ga1, threads1, L.pad1, st, P.g0,
                               s0, P.ab, h, w, radius, c.eps_f, c.eps_small, P.seg_rows1, P.colour,
                               P.gs, 3, L.geo1.hl, L.geo1.out_w, xo, nullptr, no_rag);
    } else {
        hipLaunchKernelGGL((gf_stage1_kernel<1, 1, MODE, EXACT, GREY>), ga1, threads1, L.pad1, st, P.g0, s0,
                           P.ab, h, w, radius, c.eps_f, c.eps_small, P.seg_rows1, P.colour, P.gs, 1,
                           L.geo1.hl, L.geo1.out_w, xo, nullptr, no_rag);
    }
}

void gf_part_stage1(const GfCall &c, const Part &P, int it)
{
    if (debug_get(kDbgGfExpSkip) & 1)
        ;  // timing experiment: no stage 1 (results wrong)
    else if (c.grey)  // (no exact rows, no guide cache: refused by the entry)
        launch_stage1<kS1Full, false, true>(c, P, it);
    else if (c.L.exact)
        launch_stage1<kS1Full, true, false>(c, P, it);
    else if (!c.L.keep_gs)
        launch_stage1<kS1Full, false, false>(c, P, it);
    else if (it == 0)
        launch_stage1<kS1Keep, false, false>(c, P, it);
    else
        launch_stage1<kS1Reuse, false, false>(c, P, it);
}

void gf_part_stage2(const GfCall &c, const Part &P, int it)
{
    const GfLayout &L = c.L;
    hipStream_t st = P.st;
    const int m = P.m, h = c.h, w = c.w, radius = c.radius, src_cn = c.src_cn, np = c.np;
    if (L.fused) {
        GfExact xr = {nullptr, nullptr, nullptr, 0, 0};
        if (L.exact) {
            // the rows that fail the exactness test: flagged for the column walk, listed for the row walk
            (void)hipMemsetAsync(P.xcount, 0, sizeof(int) * (size_t)m * src_cn * (1 + L.mask_words), st);
            hipLaunchKernelGGL(gf_exact_rows_kernel<0>, dim3((unsigned)ceil_div(h, 256), (unsigned)(m * src_cn)),
                               dim3(256), 0, st, P.xstat, h, L.xslots, L.geo1.strips * 8, L.geo3.strips * 8,
                               src_cn, debug_get(kDbgGfExactAllFlagged) ? -1 : gf_exact_limit(radius),
                               P.colour, P.rowmask, L.mask_words, P.xlist, P.xcount);
            xr = GfExact{P.rowmask, P.xlist, P.xcount, L.mask_words, 1};
        }
        const GfFusedArgs fa = {P.ab, P.rows, P.g0, P.d0, m, h, w, c.nb, src_cn, P.colour, st, P.xc,
                                debug_get(kDbgGfExpSkip),
                                it + 1 < c.iterations ? P.cmp : nullptr, L.lay, xr, P.cmp3,
                                // colour images (which leave the walk as planes): an XCD walks its (pair,
                                // channel) items in runs of 64 pairs per channel - a channel's
                                // neighbouring blocks then stay neighbours in time and find each other's
                                // operands in the L2 (81.6 against 82.8 ms per colour chain).  Without
                                // the planes (no room in the workspace, "gf_no_compact") the walk
                                // stores single bytes into the interleaved dst, where the three
                                // channels of a block want to run side by side (channel fastest: 0).
                                // Debug option "gf_cw_chan_run": n + 1 forces runs of n (1: channel fastest)
                                P.cmp3 != nullptr
                                    ? (debug_get(kDbgGfCwChanRun) ? debug_get(kDbgGfCwChanRun) - 1 : 64)
                                    : 0,
                                c.gcn};
        L.fused_launch(fa);
        if (P.cmp3 != nullptr && it + 1 == c.iterations && !(debug_get(kDbgGfExpSkip) & 4))
            hipLaunchKernelGGL(gf_interleave3_kernel, dim3(c.probe_blocks, m), dim3(256), 0, st, P.cmp3,
                               P.d0, c.npx, P.colour);
        return;
    }
    const int row_blocks = ceil_div(h, kBRows);
    hipLaunchKernelGGL(gf_rowsum_kernel<4>, dim3((unsigned)(m * np * row_blocks)), dim3(64), 0,
                       st, P.ab, P.rows, h, w, radius, row_blocks, np, P.colour, np);
    dim3 gc(ceil_div(w, 64), 1, m);
    if (src_cn == 3) {
        hipLaunchKernelGGL((gf_colsum_apply_kernel<3, 3>), gc, dim3(64, 12), 0, st, P.rows,
                           P.g0, P.d0, h, w, radius, P.colour, c.gcn);
        hipLaunchKernelGGL((gf_colsum_apply_kernel<1, 3>), gc, dim3(64, 4), 0, st, P.rows,
                           P.g0, P.d0, h, w, radius, P.colour, c.gcn);
    } else {
        hipLaunchKernelGGL((gf_colsum_apply_kernel<1, 1>), gc, dim3(64, 4), 0, st, P.rows,
                           P.g0, P.d0, h, w, radius, P.colour, c.gcn);
    }
}

// a whole part, step after step, on one stream
void gf_run_part(const GfCall &c, int i0, int m, int m_fill, char *ws, hipStream_t st)
{
    Part P{};
    P.i0 = i0, P.m = m, P.ws = ws, P.st = st;
    gf_part_setup(c, P, m_fill);
    gf_part_probe(c, P);
    for (int it = 0; it < c.iterations; it++) {
        gf_part_stage1(c, P, it);
        gf_part_stage2(c, P, it);
    }
}

struct SideHold {  // the entry stays ours until every launch of this call is enqueued
    hipStream_t s;
    ~SideHold() { gf_side_release(s); }
};
struct Events {  // destroyed on every path out (a pending event is released on completion)
    std::vector<hipEvent_t> ev;
    hipEvent_t make()
    {
        hipEvent_t e = nullptr;
        if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess)
            return nullptr;
        ev.push_back(e);
        return e;
    }
    ~Events()
    {
        for (hipEvent_t e : ev)
            (void)hipEventDestroy(e);
    }
};

// The staggered schedule of a forked chunk of m images from i0 (see gf_u8_entry): parts alternate
// between the two streams; stage 1 of (pass, part) waits for stage 1 of its predecessor in that
// order, which runs on the other stream
int gf_run_staggered(const char *fn, const GfCall &c, int i0, int m, char *ws0, hipStream_t stream,
                     hipStream_t side, Events &evs)
{
    int nparts = debug_get(kDbgGfParts) > 0 ? debug_get(kDbgGfParts) : 2;
    nparts = std::max(2, std::min(std::min(nparts, 16), m)) & ~1;
    std::vector<Part> parts((size_t)nparts);
    int at = 0;
    for (int p = 0; p < nparts; p++) {
        Part &P = parts[(size_t)p];
        P = Part{};
        P.i0 = i0 + at;
        P.m = m / nparts + (p < m % nparts ? 1 : 0);
        P.ws = ws0 + (size_t)at * c.L.per_img_used;
        P.st = (p & 1) ? side : stream;
        at += P.m;
        gf_part_setup(c, P, P.m);
        gf_part_probe(c, P);
    }
    hipEvent_t prev = nullptr;
    for (int it = 0; it < c.iterations; it++)
        for (int p = 0; p < nparts; p++) {
            const Part &P = parts[(size_t)p];
            if (prev != nullptr)
                RF_HIP_CHECK(hipStreamWaitEvent(P.st, prev, 0));
            gf_part_stage1(c, P, it);
            prev = evs.make();
            if (!prev)
                return fail(RF_E_HIP, "%s: hipEventCreate failed", fn);
            RF_HIP_CHECK(hipEventRecord(prev, P.st));
            gf_part_stage2(c, P, it);
        }
    return RF_OK;
}

int gf_u8_entry(const char *fn, const uint8_t *guide, const uint8_t *src, uint8_t *dst, int n, int h,
                int w, int guide_cn, int src_cn, int radius, double eps, int iterations, int flags,
                void *workspace, size_t workspace_bytes, void *stream_)
{
    if (int bad = gf_check_flags(fn, flags))
        return bad;
    if (n == 0)  // an empty batch is valid whatever the (possibly NULL) pointers are
        return RF_OK;
    if (!guide || !src || !dst || !workspace)
        return fail(RF_E_BADARG, "%s: NULL pointer", fn);
    if (n < 0 || h <= 0 || w <= 0 || iterations < 1)
        return fail(RF_E_BADARG, "%s: bad size n=%d h=%d w=%d iterations=%d", fn, n, h, w,
                    iterations);
    // a grey guide (RF_GF_GREY_AS_BGR): one byte per pixel that stands for three equal channels
    const bool grey = (flags & RF_GF_GREY_AS_BGR) != 0;
    const int gcn = grey ? 1 : 3;  // guide bytes per pixel
    if (int bad = gf_check_guide(fn, guide_cn, grey))
        return bad;
    if (int bad = gf_check_src_cn(fn, src_cn))
        return bad;
    if (int bad = gf_check_radius(fn, radius))
        return bad;
    if (int bad = gf_check_width(fn, w))
        return bad;
    if (int bad = gf_check_overlap(fn, guide, src, dst, (size_t)n * h * w, gcn, src_cn, 1))
        return bad;
    if (int bad = gf_check_grey_debug(fn, grey))
        return bad;
    if (radius > kGfMaxRadiusU8)
        return gf_via_f32(fn, guide, src, dst, n, h, w, src_cn, radius, eps, iterations, grey, workspace,
                          workspace_bytes, stream_);
    GfCall c{};
    c.guide = guide, c.src = src, c.dst = dst;
    c.h = h, c.w = w, c.src_cn = src_cn, c.radius = radius, c.iterations = iterations;
    c.grey = grey, c.gcn = gcn;
    c.np = 4 * src_cn, c.nb = ceil_div(w, kSB), c.npx = (size_t)h * w;
    c.eps_f = (float)eps;
    c.eps_small = eps < 1e-2;
    if (int bad = gf_layout(fn, n, h, w, src_cn, radius, iterations, grey, workspace_bytes, &c.L))
        return bad;
    const GfLayout &L = c.L;
    hipStream_t stream = (hipStream_t)stream_;
    // 3-channel sources: find the images whose channels are identical (see the file header)
    if (src_cn == 3) {
        c.colour_all = reinterpret_cast<int *>(workspace);
        RF_HIP_CHECK(hipMemsetAsync(c.colour_all, 0, sizeof(int) * (size_t)n, stream));
    }
    c.probe_blocks = (int)std::min<size_t>(1024, (c.npx / 4 + 255) / 256 + 1);

    // A chunk of eight or more images runs as parts on two streams - the caller's and a side
    // stream of the library, forked and joined with events, so the call still looks stream-ordered
    // to the caller and can be captured into a graph.  The kernels of a pass are bound by different
    // things (stage 1: the issue rate of its 4-cycle VALU instructions; row states: the latency of
    // a chunk of loads; column walk: memory bandwidth).
    //   aligned schedule (debug option "gf_stagger" = 0): two halves, each running its passes on its
    //       own stream from the same instant: both are in stage 1 together, then both in the walks -
    //       the second stream fills launch tails, nothing else.
    //   staggered schedule ("gf_stagger" = 1): the stage-1 launches of the parts are chained by
    //       events in the order (pass, part), parts alternating between the streams, so that at any
    //       time one part is in its VALU-bound stage 1 and the other stream's part in its
    //       memory-bound walks.  Events only: stream-ordered for the caller, capturable.
    // The debug option "gf_one_stream" keeps everything on the caller's stream,
    // "gf_force_two_streams" forks from two images on (cross-checks; identical bytes).
    char *ws0 = static_cast<char *>(workspace) + gf_header_bytes(n);
    hipStream_t side = nullptr;
    // (tools/gf_stream_sweep.py, 3 passes at 4K, two streams over one: grey 1.10 / 1.18 / 1.00 /
    //  0.93 / 0.92 / 0.87 / 0.91 and colour 0.99 / 0.97 / 0.91 / 0.93 / 0.91 / 0.89 / 0.89 at 2 / 4 /
    //  8 / 12 / 16 / 24 / 36 images: small grey launches leave XCDs idle when halved)
    const int fork_from = debug_get(kDbgGfForceTwoStreams) ? 2 : 8;
    if (L.fused && L.chunk >= fork_from && !debug_get(kDbgGfOneStream))
        side = gf_side_stream(stream);
    SideHold side_hold{side};
    const int stagger = debug_get(kDbgGfStagger);
    for (int i0 = 0; i0 < n; i0 += L.chunk) {
        const int m = std::min(L.chunk, n - i0);
        if (side == nullptr || m < fork_from) {
            gf_run_part(c, i0, m, m, ws0, stream);
            continue;
        }
        Events evs;
        hipEvent_t fork = evs.make(), join = evs.make();
        if (!fork || !join)
            return fail(RF_E_HIP, "%s: hipEventCreate failed", fn);
        RF_HIP_CHECK(hipEventRecord(fork, stream));
        RF_HIP_CHECK(hipStreamWaitEvent(side, fork, 0));
        if (!stagger) {
            const int ma = (m + 1) / 2;
            gf_run_part(c, i0, ma, m, ws0, stream);
            gf_run_part(c, i0 + ma, m - ma, m, ws0 + (size_t)ma * L.per_img_used, side);
        } else if (int bad = gf_run_staggered(fn, c, i0, m, ws0, stream, side, evs)) {
            return bad;
        }
        RF_HIP_CHECK(hipEventRecord(join, side));
        RF_HIP_CHECK(hipStreamWaitEvent(stream, join, 0));
    }
    RF_HIP_CHECK(hipGetLastError());
    return RF_OK;
}
}  // namespace

extern "C" int rf_gf_u8(const uint8_t *guide, const uint8_t *src, uint8_t *dst, int n, int h,
                        int w, int guide_cn, int src_cn, int radius, double eps, int iterations,
                        void *workspace, size_t workspace_bytes, void *stream_)
{
    return gf_u8_entry("rf_gf_u8", guide, src, dst, n, h, w, guide_cn, src_cn, radius, eps, iterations,
                       0, workspace, workspace_bytes, stream_);
}

extern "C" int rf_gf_ex_u8(const uint8_t *guide, const uint8_t *src, uint8_t *dst, int n, int h,
                           int w, int guide_cn, int src_cn, int radius, double eps, int iterations,
                           int flags, void *workspace, size_t workspace_bytes, void *stream_)
{
    return gf_u8_entry("rf_gf_ex_u8", guide, src, dst, n, h, w, guide_cn, src_cn, radius, eps,
                       iterations, flags, workspace, workspace_bytes, stream_);
}

// ------------------------------------------------------------------------------------------
// Ragged form (rf_gf_ragged_u8): images of different sizes packed one after another.
//   ragged route    one src channel, radius 1..kGfMaxRadiusU8, every image below 2^28 pixels, none of
//                   the switches that ask for another stage-2 form or a timing experiment: three
//                   launches per pass over all images (stage 1, row states, column walk), addressed
//                   through the table of rf_gf_fused.hpp, on the caller's stream alone
//   fallback route  everything else: rf_gf_ex_u8 once per image
// Workspace of the ragged route: [table, rounded up to 256 B][row states: double[4][nb_i][h_i] per
// image][alpha/beta: 16 B per pixel]; table = one GfRagImg per image, then the GfRagItem records of
// stage 1 (one per image, strip and segment; segment-major), of the row walk (one per image and 64-row
// block) and of the column walk (8 runs of ceil(blocks / 8) records, one per image and 16-column
// block in list order, the last run padded with img = -1).
// ------------------------------------------------------------------------------------------
namespace {
struct GfRaggedPlan {
    bool ragged = false;
    size_t px = 0;             // pixels of all images
    size_t state_doubles = 0;  // row states of all images
    size_t table_bytes = 0;    // image records + item records, rounded up to 256
    size_t bytes = 0;          // the workspace the route needs
    int hl = 0, out_w = 0;     // stage-1 strip geometry (the radius's and the guide kind's)
    int cw_per_xcd = 0;        // column-walk items per XCD run
    std::vector<GfRagImg> img;
    std::vector<GfRagItem> s1, rs, cw;
};

// The refusals of rf_gf_ex_u8 that need no pointers, for a list.  *px = pixels of all images.
int gf_ragged_check(const char *who, int n, const int *heights, const int *widths, int guide_cn,
                    int src_cn, int radius, int flags, size_t *px)
{
    *px = 0;
    if (int bad = gf_check_flags(who, flags))
        return bad;
    if (n < 0)
        return fail(RF_E_BADARG, "%s: bad size n=%d", who, n);
    if (!heights || !widths)
        return fail(RF_E_BADARG, "%s: NULL size array", who);
    for (int i = 0; i < n; i++) {
        if (heights[i] <= 0 || widths[i] <= 0)
            return fail(RF_E_BADARG, "%s: bad size of image %d: h=%d w=%d", who, i, heights[i],
                        widths[i]);
        *px += (size_t)heights[i] * widths[i];
        if (*px > ((size_t)1 << 58))
            return fail(RF_E_BADARG, "%s: the images hold too many pixels", who);
    }
    const bool grey = (flags & RF_GF_GREY_AS_BGR) != 0;
    if (int bad = gf_check_guide(who, guide_cn, grey))
        return bad;
    if (int bad = gf_check_src_cn(who, src_cn))
        return bad;
    if (int bad = gf_check_radius(who, radius))
        return bad;
    for (int i = 0; i < n; i++)
        if (int bad = gf_check_width(who, widths[i], i))
            return bad;
    return gf_check_grey_debug(who, grey);
}

// The route of a checked list (n > 0) and, for the ragged route, its table.
int gf_ragged_plan(const char *who, int n, const int *heights, const int *widths, int guide_cn,
                   int src_cn, int radius, int flags, GfRaggedPlan *plan)
{
    const bool grey = (flags & RF_GF_GREY_AS_BGR) != 0;
    bool ragged = src_cn == 1 && radius >= 1 && radius <= kGfMaxRadiusU8 &&
                  gf_fused_launcher(radius) != nullptr &&  // (a development build holds one radius)
                  !debug_get(kDbgGfTwoKernel) && !debug_get(kDbgGfChained) && !debug_get(kDbgGfExact) &&
                  !debug_get(kDbgGfGuideCache) &&
                  // (switches whose effect only the uniform entry implements: identical bytes either way)
                  !debug_get(kDbgGfExpSkip) && !debug_get(kDbgGfS1Cap) && !debug_get(kDbgGfS1LegacyStrips);
    for (int i = 0; i < n && ragged; i++)
        ragged = (size_t)heights[i] * widths[i] < ((size_t)1 << 28);
    plan->ragged = ragged;
    if (!ragged) {
        // rf_gf_ex_u8 once per image, on a workspace that holds the most demanding one
        size_t need = 0;
        for (int i = 0; i < n; i++)
            need = std::max(need, rf_gf_workspace_bytes(1, heights[i], widths[i], guide_cn, src_cn, radius));
        plan->bytes = need;
        return RF_OK;
    }
    // strip geometry, one for the launch: the uniform rule on the list's strip count - the halo of a
    // whole wave on either side where it costs the list no strip, else the widest strip the radius
    // allows (strip widths cannot change a byte either)
    StripGeom g0 = gf_strip_geometry(radius, 1, 1, grey);
    {
        const StripGeom gn = gf_strip_geometry(radius, 1 << 26, 1, grey);
        long long s0 = 0, sn = 0;
        for (int i = 0; i < n; i++) {
            s0 += ceil_div(widths[i], g0.out_w);
            sn += ceil_div(widths[i], gn.out_w);
        }
        if (sn < s0)
            g0 = gn;
    }
    plan->hl = g0.hl;
    plan->out_w = g0.out_w;
    plan->img.resize((size_t)n);
    size_t px0 = 0, st0 = 0, blocks = 0;
    for (int i = 0; i < n; i++) {
        const int h = heights[i], w = widths[i];
        GfRagImg &I = plan->img[(size_t)i];
        I = GfRagImg{};
        I.px0 = px0;
        I.st0 = st0;
        I.h = h;
        I.w = w;
        I.nb = ceil_div(w, kSB);
        I.strips = ceil_div(w, g0.out_w);
        // rows per segment: the uniform rule for this image as if the list held nothing but images of
        // its size - m_fill = list pixels / image pixels of them in flight together (segment lengths
        // cannot change a byte: the window sums are exact integers in any order)
        const size_t fill = std::max<size_t>(1, (plan->px + (size_t)h * w / 2) / ((size_t)h * w));
        const int m_fill = (int)std::min<size_t>(fill, 1 << 20);
        I.seg_rows = gf_pick_seg(h, radius, I.strips, m_fill, m_fill, 960, h, 4);
        I.segs = ceil_div(h, I.seg_rows);
        for (int sg = 0; sg < I.segs; sg++)
            for (int st = 0; st < I.strips; st++)
                plan->s1.push_back(GfRagItem{i, st, sg, 0});
        for (int rb = 0; rb < ceil_div(h, kBRows); rb++)
            plan->rs.push_back(GfRagItem{i, rb, 0, 0});
        for (int b = 0; b < I.nb; b++)
            plan->cw.push_back(GfRagItem{i, b, 0, 0});
        px0 += (size_t)h * w;
        st0 += (size_t)4 * I.nb * h;
        blocks += (size_t)I.nb;
    }
    // stage 1 and the row states: 256 threads per item; the column walk: 128 per block, rounded up to 8 runs
    if (!launch_fits(plan->s1.size(), stage1_threads(1)) || !launch_fits(plan->rs.size(), 256) ||
        !launch_fits(blocks + 8, 128))
        return fail(RF_E_UNSUPPORTED, "%s: too many work items for one launch", who);
    // column walk: each XCD (workgroup id mod 8) takes a contiguous run of ceil(blocks / 8) items in
    // list order - balanced by count, not by walk length
    plan->cw_per_xcd = (int)((blocks + 7) / 8);
    plan->cw.resize((size_t)plan->cw_per_xcd * 8, GfRagItem{-1, 0, 0, 0});
    plan->state_doubles = st0;
    plan->table_bytes = (plan->img.size() * sizeof(GfRagImg) +
                         (plan->s1.size() + plan->rs.size() + plan->cw.size()) * sizeof(GfRagItem) + 255) &
                        ~(size_t)255;
    plan->bytes = plan->table_bytes + plan->state_doubles * sizeof(double) + plan->px * 16;
    return RF_OK;
}

// Stage 1 of one pass over the whole list: one workgroup per item of rag.items
template <bool GREY>
void launch_ragged_stage1(const GfRaggedPlan &plan, const GfRagged rag, const uint8_t *guide,
                          const uint8_t *s0, float *ab, int radius, float eps_f, int eps_small,
                          hipStream_t stream)
{
    const GfExactOut no_xo = {nullptr, nullptr, 0, 0};
    hipLaunchKernelGGL((gf_stage1_kernel<1, 1, kS1Full, false, GREY, true>), dim3((unsigned)plan.s1.size()),
                       dim3(stage1_threads(1, GREY)), 0, stream, guide, s0, ab, 0, 0, radius, eps_f,
                       eps_small, 0, (const int *)nullptr, (float *)nullptr, 1, plan.hl, plan.out_w, no_xo,
                       (const uint8_t *)nullptr, rag);
}
}  // namespace

extern "C" size_t rf_gf_ragged_workspace_bytes(int n, const int *heights, const int *widths,
                                               int guide_cn, int src_cn, int radius, int flags)
{
    const char *who = "rf_gf_ragged_workspace_bytes";
    GfRaggedPlan plan;
    if (n <= 0 || gf_ragged_check(who, n, heights, widths, guide_cn, src_cn, radius, flags, &plan.px) != RF_OK ||
        gf_ragged_plan(who, n, heights, widths, guide_cn, src_cn, radius, flags, &plan) != RF_OK)
        return 0;
    return plan.bytes;
}

extern "C" int rf_debug_gf_launch_chunk(int chunk, int h, int w, int src_cn, int float_kernels)
{
    if (chunk < 0 || h <= 0 || w <= 0 || (src_cn != 1 && src_cn != 3))
        return rf::fail(RF_E_BADARG, "rf_debug_gf_launch_chunk: bad chunk=%d h=%d w=%d src_cn=%d", chunk, h, w,
                        src_cn);
    return rf::gf_launch_chunk(std::min(chunk, float_kernels ? rf::kMaxGridYZ : 16383), h, w, src_cn,
                               float_kernels != 0);
}

extern "C" int rf_debug_gf_ragged_plan(int n, const int *heights, const int *widths, int guide_cn,
                                       int src_cn, int radius, int flags, int *out, int cap)
{
    const char *who = "rf_debug_gf_ragged_plan";
    if (cap < 0 || (cap > 0 && !out))
        return fail(RF_E_BADARG, "%s: bad cap=%d", who, cap);
    GfRaggedPlan plan;
    if (int bad = gf_ragged_check(who, n, heights, widths, guide_cn, src_cn, radius, flags, &plan.px))
        return bad;
    if (n == 0)
        return 0;
    if (int bad = gf_ragged_plan(who, n, heights, widths, guide_cn, src_cn, radius, flags, &plan))
        return bad;
    if (!plan.ragged)
        return 0;
    const int record[6] = {3, (int)plan.s1.size(), (int)plan.rs.size(), 8 * plan.cw_per_xcd, plan.hl,
                           plan.out_w};
    std::copy(record, record + std::min(cap, 6), out);
    return 1;
}

extern "C" int rf_gf_ragged_u8(const uint8_t *guide, const uint8_t *src, uint8_t *dst, int n,
                               const int *heights, const int *widths, int guide_cn, int src_cn,
                               int radius, double eps, int iterations, int flags, void *workspace,
                               size_t workspace_bytes, void *stream_)
{
    const char *who = "rf_gf_ragged_u8";
    // (the flags first, as in rf_gf_ex_u8: an empty list with an unknown flag is refused; gf_ragged_check
    //  tests them again, after the pointers and `iterations`)
    if (int bad = gf_check_flags(who, flags))
        return bad;
    if (n == 0)  // an empty list is valid whatever the (possibly NULL) pointers are
        return RF_OK;
    if (!guide || !src || !dst)
        return fail(RF_E_BADARG, "%s: NULL image pointer", who);
    if (iterations < 1)
        return fail(RF_E_BADARG, "%s: bad iterations=%d", who, iterations);
    GfRaggedPlan plan;
    if (int bad = gf_ragged_check(who, n, heights, widths, guide_cn, src_cn, radius, flags, &plan.px))
        return bad;
    const bool grey = (flags & RF_GF_GREY_AS_BGR) != 0;
    const int gcn = grey ? 1 : 3;
    if (int bad = gf_check_overlap(who, guide, src, dst, plan.px, gcn, src_cn, 1))
        return bad;
    if (int bad = gf_ragged_plan(who, n, heights, widths, guide_cn, src_cn, radius, flags, &plan))
        return bad;
    if (!workspace || workspace_bytes < plan.bytes || ((uintptr_t)workspace & 15))
        return fail(RF_E_BADARG, "%s: workspace of %zu bytes, %zu needed (16-byte aligned)", who,
                    workspace ? workspace_bytes : (size_t)0, plan.bytes);
    hipStream_t stream = (hipStream_t)stream_;
    if (stream_is_capturing(stream))
        return fail(RF_E_UNSUPPORTED, "%s: synchronises its stream and cannot be captured into a "
                                      "graph", who);
    if (!plan.ragged) {
        size_t first = 0;
        for (int i = 0; i < n; i++) {
            const int rc = rf_gf_ex_u8(guide + first * gcn, src + first * src_cn, dst + first * src_cn,
                                       1, heights[i], widths[i], guide_cn, src_cn, radius, eps,
                                       iterations, flags, workspace, workspace_bytes, stream_);
            if (rc != RF_OK)
                return rc;
            first += (size_t)heights[i] * widths[i];
        }
        return RF_OK;
    }
    // ---- the table: image records, then the item records of the three kernels, one copy --------
    const size_t n_img = plan.img.size(), n_s1 = plan.s1.size(), n_rs = plan.rs.size(),
                 n_cw = plan.cw.size();
    std::vector<unsigned char> image(n_img * sizeof(GfRagImg) + (n_s1 + n_rs + n_cw) * sizeof(GfRagItem));
    unsigned char *at = image.data();
    __builtin_memcpy(at, plan.img.data(), n_img * sizeof(GfRagImg));
    at += n_img * sizeof(GfRagImg);
    __builtin_memcpy(at, plan.s1.data(), n_s1 * sizeof(GfRagItem));
    at += n_s1 * sizeof(GfRagItem);
    __builtin_memcpy(at, plan.rs.data(), n_rs * sizeof(GfRagItem));
    at += n_rs * sizeof(GfRagItem);
    __builtin_memcpy(at, plan.cw.data(), n_cw * sizeof(GfRagItem));
    char *ws = static_cast<char *>(workspace);
    const GfRagImg *d_img = reinterpret_cast<const GfRagImg *>(ws);
    const GfRagItem *d_s1 = reinterpret_cast<const GfRagItem *>(ws + n_img * sizeof(GfRagImg));
    const GfRagItem *d_rs = d_s1 + n_s1, *d_cw = d_rs + n_rs;
    double *states = reinterpret_cast<double *>(ws + plan.table_bytes);
    float *ab = reinterpret_cast<float *>(states + plan.state_doubles);
    // the host image must outlive the copy: the copy is waited for before the launches (this is the
    // call's one synchronisation of `stream`)
    RF_HIP_CHECK(hipMemcpyAsync(workspace, image.data(), image.size(), hipMemcpyHostToDevice, stream));
    RF_HIP_CHECK(hipStreamSynchronize(stream));
    const float eps_f = (float)eps;
    const int eps_small = eps < 1e-2;
    const GfFusedLaunch fused_launch = gf_fused_launcher(radius);
    const GfRagged rag_s1 = {d_img, d_s1};
    for (int it = 0; it < iterations; it++) {
        const uint8_t *s0 = it == 0 ? src : (const uint8_t *)dst;  // pass k reads the packed result of pass k - 1
        if (grey)
            launch_ragged_stage1<true>(plan, rag_s1, guide, s0, ab, radius, eps_f, eps_small, stream);
        else
            launch_ragged_stage1<false>(plan, rag_s1, guide, s0, ab, radius, eps_f, eps_small, stream);
        GfFusedArgs fa = {};
        fa.ab = ab;
        fa.states = states;
        fa.guide = guide;
        fa.dst = dst;
        fa.src_cn = 1;
        fa.stream = stream;
        fa.guide_cn = gcn;
        fa.rag_rs = GfRagged{d_img, d_rs};
        fa.rag_cw = GfRagged{d_img, d_cw};
        fa.rs_items = (int)n_rs;
        fa.cw_per_xcd = plan.cw_per_xcd;
        fa.rag_ab_bytes = plan.px * 16;
        fused_launch(fa);
    }
    RF_HIP_CHECK(hipGetLastError());
    return RF_OK;
}

