// rf_jbf_points.hip -- the joint bilateral filter evaluated at listed pixels only, for many
// parameter sets in one launch (rf_jbf_points_u8): the bilateral half of a WHDR parameter sweep.
//
// An output pixel of rf_jbf_u8 depends only on its own disk, so the bytes at a few hundred
// judgement points per image can be computed directly, with the per-pixel arithmetic of
// jbf_generic_kernel (rf_jbf.hip): taps in the d_di / d_dj order, w = sw[k] * lut[sad],
// separately rounded multiply and add, sum * (1 / wsum) unless true division is asked for.
//
// Mapping: the parameter sets are grouped by sigma_space (one tap table, one radius per group)
// and each group is cut into chunks of at most 64 sets.  A wave works on one chunk: its lanes are
// (point, set) pairs, up to 64 / nsets points per wave (fewer while the launch would have under
// 4096 waves), so every lane of a point reads the same texel
// per tap (a broadcast) and the tap offsets and spatial weights are wave-uniform (scalar loads);
// only the colour-table read differs per lane.  The tables are interleaved [sad][set] per chunk, so
// the lanes of one point read neighbouring words.  Every output is one sequential chain over its
// disk (no reduction across lanes: the summation order is the contract).  Chunks are issued in
// order of decreasing radius, so the long chains start first.
//
// Tables: built on the host by the functions rf_jbf_u8's own cache uses, under rf_jbf_u8's argument
// rules (both in rf_jbf_common.hpp), staged into the caller's workspace with one copy per call; the
// library's table cache (rf_jbf_tables.hip) is not touched.
//
// Ragged form (rf_jbf_points_ragged_u8): the images of a call may differ in size and lie packed one
// after another.  Every lane already finds its image by a binary search over point_offsets and
// reads single texels, so the only difference is where the image's first pixel, height and width
// come from: a 16-byte record per image (staged behind the tables, in the same copy) instead of
// i * h * w and the launch's h, w.  Both kernels are one lane body (jbf_points_lane<kRagged>);
// the plan, the checks and the staging are shared (points_call).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "reflectance_filtering_debug.h"
#include "rf_jbf_common.hpp"

namespace rf {
namespace {

constexpr int kPtsMaxSets = 64;  // sets per chunk = lanes of a wave
constexpr int kPtsWaves = 4;     // waves per workgroup
constexpr int kPtsUnroll = 8;    // taps whose loads are issued before the first of them is added
constexpr int kPtsMinWaves = 4096;  // waves a launch should have before lanes take several points

struct PtsChunk {
    int tap_off;     // first tap of the chunk's group in the tap table
    int maxk;        // taps of the disk
    int lut_off;     // first float of the chunk's interleaved colour tables
    int nsets;       // parameter sets of the chunk (1..64)
    int ppw;         // points per wave, 1 .. 64 / nsets
    int item_begin;  // first work item (wave) of the chunk
    int param[kPtsMaxSets];  // global index of each set
};

struct PtsGroup {
    double sigma_space;
    int radius;
    int maxk;
    std::vector<int> params;
};

// Taps of the radius-r disk: the predicate of jbf_space_taps, without the weights.
int disk_taps(int radius)
{
    long long count = 0;
    for (int i = -radius; i <= radius; i++)
        for (int j = -radius; j <= radius; j++)
            if (!(std::sqrt((double)i * i + (double)j * j) > radius))
                count++;
    return (int)count;
}

// One chunk of the launch plan: sets [first, first + nsets) of a group, in launch order.
struct PtsPlanChunk {
    int group;        // index into PtsPlan::groups
    int first;        // first set of the chunk within the group's params
    int nsets;        // parameter sets of the chunk (1..64)
    int ppw;          // points per wave, 1 .. 64 / nsets
    long long waves;  // work items of the chunk: ceil(total_points / ppw)
};

struct PtsPlan {
    std::vector<PtsGroup> groups;  // in launch order: decreasing radius
    std::vector<PtsPlanChunk> chunks;  // in launch order
    int nchunks = 0;
    long long items = 0;           // waves of the launch (the sum over the chunks)
    size_t taps = 0;               // entries of the tap table
    size_t lut_floats = 0;
    size_t off_chunks = 0, off_taps = 0, off_luts = 0, bytes = 0;
};

inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

// Groups, chunks with their points per wave, sizes and the workspace layout [chunks][taps][luts]
// of one call of total_points points: the one place that decides what rf_jbf_points_u8 launches
// (rf_debug_jbf_points_plan reports it).  Host only.  Fails on a radius rf_jbf_u8 refuses.
int plan_points(const char *who, int n_params, const double *sigma_space, int d, int nlut,
                int total_points, PtsPlan *plan)
{
    for (int p = 0; p < n_params; p++) {
        const double ss = jbf_sigma(sigma_space[p]);
        PtsGroup *g = nullptr;
        for (PtsGroup &e : plan->groups)
            if (e.sigma_space == ss)
                g = &e;
        if (!g) {
            const int radius = jbf_radius(d, ss);
            if (radius > kJbfMaxRadius)
                return fail(RF_E_UNSUPPORTED, "%s: radius %d too large", who, radius);
            plan->groups.push_back(PtsGroup{ss, radius, 0, {}});
            g = &plan->groups.back();
        }
        g->params.push_back(p);
    }
    std::stable_sort(plan->groups.begin(), plan->groups.end(),
                     [](const PtsGroup &a, const PtsGroup &b) { return a.radius > b.radius; });
    for (PtsGroup &g : plan->groups) {
        g.maxk = disk_taps(g.radius);
        plan->taps += (size_t)g.maxk;
        plan->nchunks += ((int)g.params.size() + kPtsMaxSets - 1) / kPtsMaxSets;
        plan->lut_floats += (size_t)nlut * g.params.size();
    }
    if (plan->taps > (size_t)0x7fffffff || plan->lut_floats > (size_t)0x7fffffff)
        return fail(RF_E_UNSUPPORTED, "%s: tables too large for one call", who);
    plan->off_chunks = 0;
    plan->off_taps = align256(sizeof(PtsChunk) * plan->nchunks);
    plan->off_luts = plan->off_taps + align256(sizeof(uint2) * plan->taps);
    plan->bytes = plan->off_luts + align256(sizeof(float) * plan->lut_floats);
    for (size_t gi = 0; gi < plan->groups.size(); gi++) {
        const size_t gsets = plan->groups[gi].params.size();
        for (size_t first = 0; first < gsets; first += kPtsMaxSets) {
            PtsPlanChunk pc;
            pc.group = (int)gi;
            pc.first = (int)first;
            pc.nsets = (int)std::min(gsets - first, (size_t)kPtsMaxSets);
            // points per wave: as many as the lanes hold once the launch has enough waves to
            // fill the chip; below that, fewer (down to one), so that short lists still spread
            // their chains over many waves (a chain is latency-bound, lanes are not the limit)
            pc.ppw = std::max(1, std::min(kPtsMaxSets / pc.nsets,
                                          (int)(((long long)total_points * plan->nchunks) /
                                                kPtsMinWaves)));
            pc.waves = ((long long)total_points + pc.ppw - 1) / pc.ppw;
            plan->items += pc.waves;
            plan->chunks.push_back(pc);
        }
    }
    return RF_OK;
}

// One launch of kPtsWaves waves per workgroup takes every item (a wave each).
bool plan_fits_one_launch(const PtsPlan &plan)
{
    return launch_fits((unsigned long long)(plan.items + kPtsWaves - 1) / kPtsWaves, 64 * kPtsWaves);
}

// One image of a ragged call (rf_jbf_points_ragged_u8): where its pixels start in the packed
// buffers, and its size.
struct alignas(16) PtsImage {
    long long first;  // pixels before the image: the sum of h * w of the images in front of it
    int h, w;
};
static_assert(sizeof(PtsImage) == 16, "the workspace holds 16 bytes per image");

// One wave = one work item = up to 64 (point, set) lanes of one chunk.  The lane body of both
// kernels: with kRagged the image's first pixel and size come from images[i] of the image the
// lane's point belongs to (they differ between the lanes of a wave once ppw > 1), without it
// every image is h x w (wave-uniform kernel arguments) and `images` is not read.
template <bool kRagged>
__device__ __forceinline__ void jbf_points_lane(
    const uint8_t *__restrict__ joint, const uint8_t *__restrict__ src, uint8_t *__restrict__ out,
    int n, int h, int w, const PtsImage *__restrict__ images, int jcn, int scn, int border,
    int flags, const int *__restrict__ points, const int *__restrict__ point_offsets, int total,
    const PtsChunk *__restrict__ chunks, int nchunks, const uint2 *__restrict__ taps,
    const float *__restrict__ luts, int items)
{
    const int item = __builtin_amdgcn_readfirstlane(blockIdx.x * kPtsWaves + (threadIdx.x >> 6));
    if (item >= items)
        return;
    // the chunk: last one with item_begin <= item (wave-uniform)
    int lo = 0, hi = nchunks - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (chunks[mid].item_begin <= item)
            lo = mid;
        else
            hi = mid - 1;
    }
    const PtsChunk *ch = chunks + lo;
    const int nsets = ch->nsets;
    const int lane = threadIdx.x & 63;
    const int sub = lane / nsets, s = lane - sub * nsets;
    const int k = (item - ch->item_begin) * ch->ppw + sub;
    const bool active = sub < ch->ppw && k < total;
    // idle lanes follow point 0 through the loop (no divergence there) and write nothing.
    // Points are validated by the caller; clamping keeps every read inside the image anyway.
    const int kk = active ? k : 0;
    const int rx = points[2 * kk], ry = points[2 * kk + 1];
    int ilo = 0, ihi = n - 1;  // the image: last i with point_offsets[i] <= kk
    while (ilo < ihi) {
        const int mid = (ilo + ihi + 1) >> 1;
        if (point_offsets[mid] <= kk)
            ilo = mid;
        else
            ihi = mid - 1;
    }
    size_t img;
    if (kRagged) {
        const PtsImage im = images[ilo];
        img = (size_t)im.first;
        h = im.h;
        w = im.w;
    } else {
        img = (size_t)ilo * h * w;
    }
    const int px = min(max(rx, 0), w - 1);
    const int py = min(max(ry, 0), h - 1);
    const uint32_t j0 = load_packed(joint, img + (size_t)py * w + px, jcn);
    const float *__restrict__ lut = luts + ch->lut_off + s;  // entry a of this set: lut[a * nsets]
    const uint2 *__restrict__ tp = taps + ch->tap_off;
    const int maxk = ch->maxk;
    float sum[3] = {0.f, 0.f, 0.f};
    float wsum = 0.f;
    for (int t0 = 0; t0 < maxk; t0 += kPtsUnroll) {
        const int cnt = min(kPtsUnroll, maxk - t0);
        uint32_t jt[kPtsUnroll], st[kPtsUnroll];
        float sw[kPtsUnroll], lw[kPtsUnroll];
#pragma unroll
        for (int u = 0; u < kPtsUnroll; u++) {
            jt[u] = st[u] = 0u;
            sw[u] = 0.f;
            if (u < cnt) {
                const uint2 tap = tp[t0 + u];
                const int di = (int)tap.x >> 16;
                const int dj = (int)(int16_t)(tap.x & 0xffffu);
                sw[u] = __uint_as_float(tap.y);
                const int yy = border_interpolate(py + di, h, border);
                const int xx = border_interpolate(px + dj, w, border);
                if (yy >= 0 && xx >= 0) {
                    const size_t q = img + (size_t)yy * w + xx;
                    jt[u] = load_packed(joint, q, jcn);
                    st[u] = load_packed(src, q, scn);
                }
            }
        }
#pragma unroll
        for (int u = 0; u < kPtsUnroll; u++)
            lw[u] = u < cnt ? lut[__builtin_amdgcn_sad_u8(j0, jt[u], 0u) * nsets] : 0.f;
#pragma unroll
        for (int u = 0; u < kPtsUnroll; u++) {
            if (u < cnt) {
                const float wgt = __fmul_rn(sw[u], lw[u]);
                sum[0] = __fadd_rn(sum[0], __fmul_rn(wgt, (float)(st[u] & 0xff)));
                if (scn == 3) {
                    sum[1] = __fadd_rn(sum[1], __fmul_rn(wgt, (float)((st[u] >> 8) & 0xff)));
                    sum[2] = __fadd_rn(sum[2], __fmul_rn(wgt, (float)((st[u] >> 16) & 0xff)));
                }
                wsum = __fadd_rn(wsum, wgt);
            }
        }
    }
    if (active)
        finish_pixel(out + ((size_t)ch->param[s] * total + k) * scn, sum, wsum, scn, flags);
}

__global__ __launch_bounds__(64 * kPtsWaves) void jbf_points_kernel(
    const uint8_t *__restrict__ joint, const uint8_t *__restrict__ src, uint8_t *__restrict__ out,
    int n, int h, int w, int jcn, int scn, int border, int flags, const int *__restrict__ points,
    const int *__restrict__ point_offsets, int total, const PtsChunk *__restrict__ chunks,
    int nchunks, const uint2 *__restrict__ taps, const float *__restrict__ luts, int items)
{
    jbf_points_lane<false>(joint, src, out, n, h, w, nullptr, jcn, scn, border, flags, points,
                           point_offsets, total, chunks, nchunks, taps, luts, items);
}

// The same lanes over images of different sizes, packed one after another.
__global__ __launch_bounds__(64 * kPtsWaves) void jbf_points_ragged_kernel(
    const uint8_t *__restrict__ joint, const uint8_t *__restrict__ src, uint8_t *__restrict__ out,
    int n, const PtsImage *__restrict__ images, int jcn, int scn, int border, int flags,
    const int *__restrict__ points, const int *__restrict__ point_offsets, int total,
    const PtsChunk *__restrict__ chunks, int nchunks, const uint2 *__restrict__ taps,
    const float *__restrict__ luts, int items)
{
    jbf_points_lane<true>(joint, src, out, n, 0, 0, images, jcn, scn, border, flags, points,
                          point_offsets, total, chunks, nchunks, taps, luts, items);
}

// The colour-table length (entries per set) of a call: 256 per table channel (jbf_table_cn: 768
// for a grey joint read as three equal channels).  0 = bad channel count.
int points_nlut(int joint_cn, int flags)
{
    if (joint_cn != 1 && joint_cn != 3)
        return 0;
    return 256 * jbf_table_cn(joint_cn, flags);
}

}  // namespace
}  // namespace rf

extern "C" size_t rf_jbf_points_workspace_bytes(int n_params, const double *sigma_space, int d,
                                                int joint_cn, int flags)
{
    using namespace rf;
    const int nlut = points_nlut(joint_cn, flags);
    if (n_params <= 0 || !sigma_space || nlut == 0)
        return 0;
    PtsPlan plan;
    if (plan_points("rf_jbf_points_u8", n_params, sigma_space, d, nlut, 0, &plan) != RF_OK)
        return 0;
    return plan.bytes;
}

extern "C" int rf_debug_jbf_points_plan(int n_params, const double *sigma_space, int d,
                                        int joint_cn, int flags, int total_points, int *out,
                                        int max_chunks)
{
    using namespace rf;
    if (n_params <= 0 || !sigma_space)
        return fail(RF_E_BADARG, "rf_debug_jbf_points_plan: no parameter sets (n_params=%d)",
                    n_params);
    if (total_points < 0 || max_chunks < 0 || (max_chunks > 0 && !out))
        return fail(RF_E_BADARG, "rf_debug_jbf_points_plan: bad size total_points=%d max_chunks=%d",
                    total_points, max_chunks);
    if (joint_cn != 1 && joint_cn != 3)
        return fail(RF_E_UNSUPPORTED, "rf_debug_jbf_points_plan: joint channels must be 1 or 3 (%d)",
                    joint_cn);
    if (flags & ~kJbfPublicFlags)
        return fail(RF_E_BADARG, "rf_debug_jbf_points_plan: unknown flag bits 0x%x", flags);
    PtsPlan plan;
    const int rc = plan_points("rf_jbf_points_u8", n_params, sigma_space, d,
                               points_nlut(joint_cn, flags), total_points, &plan);
    if (rc != RF_OK)
        return rc;
    if (!plan_fits_one_launch(plan))
        return fail(RF_E_UNSUPPORTED, "rf_debug_jbf_points_plan: too many points for one launch");
    for (int c = 0; c < plan.nchunks && c < max_chunks; c++) {
        const PtsPlanChunk &pc = plan.chunks[c];
        out[4 * c + 0] = plan.groups[pc.group].radius;
        out[4 * c + 1] = pc.nsets;
        out[4 * c + 2] = pc.ppw;
        out[4 * c + 3] = (int)pc.waves;
    }
    return plan.nchunks;
}

namespace rf {
namespace {

// Both entries: rf_jbf_points_u8 (heights == nullptr: n images of h x w) and
// rf_jbf_points_ragged_u8 (heights / widths: n host ints each, images packed one after another).
// The argument checks, the plan, the table staging and the launch; `who` names the entry.
int points_call(const char *who, const uint8_t *joint, const uint8_t *src, int n, int h, int w,
                const int *heights, const int *widths, bool ragged, int joint_cn, int src_cn,
                const int *points, const int *point_offsets, int total_points, int n_params,
                const double *sigma_color, const double *sigma_space, int d, int border, int flags,
                uint8_t *out, void *workspace, size_t workspace_bytes, void *stream_)
{
    if (n == 0)
        return RF_OK;
    if (!joint || !src || !points || !point_offsets || !out || (ragged && (!heights || !widths)))
        return fail(RF_E_BADARG, "%s: NULL pointer", who);
    if (ragged) {
        if (n < 0 || total_points < 0)
            return fail(RF_E_BADARG, "%s: bad size n=%d total_points=%d", who, n, total_points);
    } else if (n < 0 || h <= 0 || w <= 0 || total_points < 0) {
        return fail(RF_E_BADARG, "%s: bad size n=%d h=%d w=%d total_points=%d", who, n, h, w,
                    total_points);
    }
    size_t px = 0;  // pixels of all images
    if (ragged) {
        for (int i = 0; i < n; i++) {
            if (heights[i] <= 0 || widths[i] <= 0)
                return fail(RF_E_BADARG, "%s: bad size of image %d: h=%d w=%d", who, i,
                            heights[i], widths[i]);
            px += (size_t)heights[i] * widths[i];
            if (px > ((size_t)1 << 60))
                return fail(RF_E_BADARG, "%s: the images hold too many pixels", who);
        }
    } else {
        px = (size_t)n * h * w;
    }
    if (n_params <= 0 || !sigma_color || !sigma_space)
        return fail(RF_E_BADARG, "%s: no parameter sets (n_params=%d)", who, n_params);
    if ((joint_cn != 1 && joint_cn != 3) || (src_cn != 1 && src_cn != 3))
        return fail(RF_E_UNSUPPORTED, "%s: channels must be 1 or 3 (joint %d, src %d)", who,
                    joint_cn, src_cn);
    if (border < 0 || border > 4)
        return fail(RF_E_UNSUPPORTED, "%s: border type %d", who, border);
    if (flags & ~kJbfPublicFlags)
        return fail(RF_E_BADARG, "%s: unknown flag bits 0x%x", who, flags);
    {
        const size_t nout = (size_t)n_params * total_points * src_cn;
        if (ranges_overlap(out, nout, joint, px * joint_cn) ||
            ranges_overlap(out, nout, src, px * src_cn))
            return fail(RF_E_BADARG, "%s: out must not overlap an input", who);
    }
    const int nlut = points_nlut(joint_cn, flags);
    const int jcn_kernel = jbf_kernel_cn(joint_cn, flags);
    PtsPlan plan;
    int rc = plan_points(who, n_params, sigma_space, d, nlut, total_points, &plan);
    if (rc != RF_OK)
        return rc;
    // a ragged call keeps its image records behind the tables: [chunks][taps][luts][images]
    const size_t off_images = plan.bytes;
    const size_t bytes = plan.bytes + (ragged ? align256(sizeof(PtsImage) * (size_t)n) : 0);
    if (!workspace || workspace_bytes < bytes)
        return fail(RF_E_WORKSPACE, "%s: workspace of %zu bytes, %zu needed", who,
                    workspace ? workspace_bytes : (size_t)0, bytes);
    hipStream_t stream = (hipStream_t)stream_;
    if (stream_is_capturing(stream))
        return fail(RF_E_UNSUPPORTED, "%s: synchronises its stream and cannot be captured into a "
                                      "graph", who);
    if (total_points == 0)
        return RF_OK;
    if (!plan_fits_one_launch(plan))
        return fail(RF_E_UNSUPPORTED, "%s: too many points for one launch", who);

    // ---- tables: one host image of the workspace, copied with one call --------------------
    std::vector<char> image(bytes, 0);
    PtsChunk *chunks = reinterpret_cast<PtsChunk *>(image.data() + plan.off_chunks);
    uint2 *taps = reinterpret_cast<uint2 *>(image.data() + plan.off_taps);
    float *luts = reinterpret_cast<float *>(image.data() + plan.off_luts);
    int tap_off = 0, lut_off = 0, item = 0;
    size_t c = 0;
    std::vector<int> di, dj, hw;
    std::vector<float> sw, lut;
    for (size_t gi = 0; gi < plan.groups.size(); gi++) {
        const PtsGroup &g = plan.groups[gi];
        jbf_space_taps(g.radius, g.sigma_space, di, dj, sw, hw);
        if ((int)di.size() != g.maxk)
            return fail(RF_E_HIP, "%s: tap count mismatch (internal)", who);
        for (int t = 0; t < g.maxk; t++) {
            taps[tap_off + t].x = ((uint32_t)di[t] << 16) | ((uint32_t)dj[t] & 0xffffu);
            uint32_t bits;
            std::memcpy(&bits, &sw[t], 4);
            taps[tap_off + t].y = bits;
        }
        for (; c < plan.chunks.size() && plan.chunks[c].group == (int)gi; c++) {
            const PtsPlanChunk &pc = plan.chunks[c];
            PtsChunk &ch = chunks[c];
            ch.tap_off = tap_off;
            ch.maxk = g.maxk;
            ch.lut_off = lut_off;
            ch.nsets = pc.nsets;
            ch.ppw = pc.ppw;
            ch.item_begin = item;
            for (int s = 0; s < ch.nsets; s++) {
                const int p = g.params[pc.first + s];
                ch.param[s] = p;
                jbf_colour_lut(nlut / 256, jbf_sigma(sigma_color[p]), lut);
                for (int a = 0; a < nlut; a++)
                    luts[lut_off + (size_t)a * ch.nsets + s] = lut[a];
            }
            lut_off += nlut * ch.nsets;
            item += (int)pc.waves;
        }
        tap_off += g.maxk;
    }
    if (ragged) {
        PtsImage *images = reinterpret_cast<PtsImage *>(image.data() + off_images);
        long long first = 0;
        for (int i = 0; i < n; i++) {
            images[i] = PtsImage{first, heights[i], widths[i]};
            first += (long long)heights[i] * widths[i];
        }
    }
    // the host image must outlive the copy: the copy is waited for before the launch (this is
    // the call's one synchronisation of `stream`)
    RF_HIP_CHECK(hipMemcpyAsync(workspace, image.data(), bytes, hipMemcpyHostToDevice, stream));
    RF_HIP_CHECK(hipStreamSynchronize(stream));
    char *ws = static_cast<char *>(workspace);
    const int blocks = (item + kPtsWaves - 1) / kPtsWaves;
    const PtsChunk *d_chunks = reinterpret_cast<const PtsChunk *>(ws + plan.off_chunks);
    const uint2 *d_taps = reinterpret_cast<const uint2 *>(ws + plan.off_taps);
    const float *d_luts = reinterpret_cast<const float *>(ws + plan.off_luts);
    if (ragged)
        hipLaunchKernelGGL(jbf_points_ragged_kernel, dim3(blocks), dim3(64 * kPtsWaves), 0, stream,
                           joint, src, out, n, reinterpret_cast<const PtsImage *>(ws + off_images),
                           jcn_kernel, src_cn, border, flags, points, point_offsets,
                           total_points, d_chunks, plan.nchunks, d_taps, d_luts, item);
    else
        hipLaunchKernelGGL(jbf_points_kernel, dim3(blocks), dim3(64 * kPtsWaves), 0, stream, joint,
                           src, out, n, h, w, jcn_kernel, src_cn, border, flags, points,
                           point_offsets, total_points, d_chunks, plan.nchunks, d_taps, d_luts,
                           item);
    RF_HIP_CHECK(hipGetLastError());
    return RF_OK;
}

}  // namespace
}  // namespace rf

extern "C" int rf_jbf_points_u8(const uint8_t *joint, const uint8_t *src, int n, int h, int w,
                                int joint_cn, int src_cn, const int *points,
                                const int *point_offsets, int total_points, int n_params,
                                const double *sigma_color, const double *sigma_space, int d,
                                int border, int flags, uint8_t *out, void *workspace,
                                size_t workspace_bytes, void *stream)
{
    return rf::points_call("rf_jbf_points_u8", joint, src, n, h, w, nullptr, nullptr, false,
                           joint_cn, src_cn, points, point_offsets, total_points, n_params,
                           sigma_color, sigma_space, d, border, flags, out, workspace,
                           workspace_bytes, stream);
}

extern "C" size_t rf_jbf_points_ragged_workspace_bytes(int n, int n_params,
                                                       const double *sigma_space, int d,
                                                       int joint_cn, int flags)
{
    const size_t tables = rf_jbf_points_workspace_bytes(n_params, sigma_space, d, joint_cn, flags);
    if (n < 0 || tables == 0)
        return 0;
    return tables + rf::align256(sizeof(rf::PtsImage) * (size_t)n);
}

extern "C" int rf_jbf_points_ragged_u8(const uint8_t *joint, const uint8_t *src, int n,
                                       const int *heights, const int *widths, int joint_cn,
                                       int src_cn, const int *points, const int *point_offsets,
                                       int total_points, int n_params, const double *sigma_color,
                                       const double *sigma_space, int d, int border, int flags,
                                       uint8_t *out, void *workspace, size_t workspace_bytes,
                                       void *stream)
{
    return rf::points_call("rf_jbf_points_ragged_u8", joint, src, n, 0, 0, heights, widths, true,
                           joint_cn, src_cn, points, point_offsets, total_points, n_params,
                           sigma_color, sigma_space, d, border, flags, out, workspace,
                           workspace_bytes, stream);
}
