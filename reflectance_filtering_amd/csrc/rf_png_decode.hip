// rf_png_decode.hip -- the device half of a PNG decode, for gfx950: the inflated IDAT streams of
// images of different sizes and formats (per row one filter byte and w * bpp filtered bytes) to
// packed 8-bit BGR images, in three launches per call.  The host inflates (image_utils.png_parse);
// what is left parallelises:
//
//   1. png_unfilter_kernel, one workgroup of 16 waves per image, undoes the row filters in place.
//      Every byte depends on its left neighbour a, the byte above b and the byte above-left c,
//      whatever the filter types of the two rows are, so the rows of a block are reconstructed as a
//      skewed wavefront: lane k works on one row at pixel x = t - k in step t.  a is the lane's own
//      result of step t - 1; b is what lane k - 1 produced in step t - 1 and c what it produced in
//      step t - 2, so one DPP wave shift per step brings b, and c is the b of the step before.  A
//      lane whose pixel is outside its row produces zeros: the zeros left of a row and above the
//      first one.  Lane 0 does not reconstruct: it walks the last row of the block before (already
//      reconstructed, taken as filter None, not stored), so that one body serves every lane - a
//      block is 63 new rows.  The lanes select by their row's filter byte; a byte above 4 counts as
//      None and sets the image's bad bit.
//        A lane reads and writes its row in groups of 8 pixels, 4 where a pixel has 6 or 8 bytes
//      (one to three unaligned dword accesses where the group lies inside the row), the next group
//      being read before the current one is computed.  The blocks of an image run as a pipeline over the workgroup's waves: a
//      super-step is one group of every active wave and a barrier; block b starts kLag super-steps
//      after block b - 1 (lag_of), when everything its lane 0 is about to read has been stored.
//      Every wave of the workgroup runs the same number of super-steps, a function of the image's
//      size alone.
//   2. png_unpack_kernel, one thread per pixel: samples to BGR (RGB swapped, grey replicated, alpha
//      dropped, the high byte of 16-bit samples, a palette index to its entry) and, per workgroup,
//      one integer OR into the image's flag word where a pixel's channels differ.
//   3. png_flags_kernel: the flag words to the n flag bytes.
//
// The bytes written are a function of the input alone: the one atomic is an integer OR.
#include <vector>

#include "rf_common.hpp"

namespace rf {
namespace {

constexpr int kRows = 63;                  // new rows per block (lane 0 re-reads the row above them)
// pixels per lane and group (steps per super-step): 32 bytes of a row at most, so that the three
// groups a lane holds (read ahead, in work, results) fit the 128 registers of a 16-wave workgroup
constexpr int group_px(int bpp) { return bpp >= 6 ? 4 : 8; }
constexpr int kWaves = 16;
constexpr int kUnfilterThreads = 64 * kWaves;
// Lane 0 of block b reads pixel x of the row above in step x; lane 63 of block b - 1 produces it in
// its step x + 63, that is in its super-step (x + 63) / kG, and stores it before that super-step's
// barrier.  Group g + 1 (pixels up to (g + 2) * kG - 1) is read in super-step g of block b, so its
// last pixel is stored in super-step g + 2 + 62 / kG of block b - 1, which has to end before:
constexpr int lag_of(int group) { return 2 + 62 / group + 1; }
constexpr int kUnpackThreads = 256;
constexpr int kUnpackPx = 4096;            // pixels per workgroup of the unpack kernel
constexpr unsigned kFlagBad = 2u, kFlagColour = 4u;   // bits of a flag word

// One image of a call.
struct DecImage {
    unsigned long long raw0;    // first byte of its stream in `raw`
    unsigned long long first;   // pixels before the image
    unsigned int h, w;
    unsigned int rowlen;        // 1 + w * bpp
    unsigned int bpp;
    unsigned int ctype;
    unsigned int sample;        // bytes per sample: 1 or 2
    unsigned int blk0;          // its first workgroup in the unpack grid
    unsigned int nblk;
};
static_assert(sizeof(DecImage) == 48, "the workspace holds 48 bytes per image");

// ---- reconstruction ------------------------------------------------------------------------------

// What lane k - 1 holds in v (lane 0: zero).  All 64 lanes have to be active.
__device__ __forceinline__ unsigned from_lane_above(unsigned v)
{
    return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x138 /* wave_shr:1 */, 0xf, 0xf, false);
}

// The kG pixels from x0 on of a row (`px` is its first sample; bytes outside the row read as zero).
template <int BPP, int kG>
__device__ __forceinline__ void load_group(const uint8_t *px, bool rowok, int x0, int w,
                                           unsigned (&buf)[kG * BPP / 4])
{
    if (rowok && x0 >= 0 && x0 + kG <= w) {
        __builtin_memcpy(buf, px + (size_t)x0 * BPP, kG * BPP);
        return;
    }
#pragma unroll
    for (int k = 0; k < kG * BPP / 4; k++)
        buf[k] = 0;
#pragma unroll
    for (int j = 0; j < kG; j++) {
        const int x = x0 + j;
        if (rowok && x >= 0 && x < w) {
            uint8_t t[BPP];
            __builtin_memcpy(t, px + (size_t)x * BPP, BPP);
#pragma unroll
            for (int i = 0; i < BPP; i++)
                buf[(j * BPP + i) >> 2] |= (unsigned)t[i] << (8 * ((j * BPP + i) & 3));
        }
    }
}

template <int BPP, int kG>
__device__ __forceinline__ void store_group(uint8_t *px, bool rowok, int x0, int w,
                                            const unsigned (&buf)[kG * BPP / 4])
{
    if (!rowok)
        return;
    if (x0 >= 0 && x0 + kG <= w) {
        __builtin_memcpy(px + (size_t)x0 * BPP, buf, kG * BPP);
        return;
    }
#pragma unroll
    for (int j = 0; j < kG; j++) {
        const int x = x0 + j;
        if (x >= 0 && x < w) {
            uint8_t t[BPP];
#pragma unroll
            for (int i = 0; i < BPP; i++)
                t[i] = (uint8_t)(buf[(j * BPP + i) >> 2] >> (8 * ((j * BPP + i) & 3)));
            __builtin_memcpy(px + (size_t)x * BPP, t, BPP);
        }
    }
}

// The rows of one image, in place.  Returns whether this lane met a filter byte above 4.
template <int BPP>
__device__ bool unfilter_image(uint8_t *raw, const int h, const int w, const unsigned rowlen)
{
    constexpr int kWords = (BPP + 3) / 4;   // dwords of one pixel
    constexpr int kG = group_px(BPP), kLag = lag_of(kG);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned blocks = ((unsigned)h + kRows - 1) / kRows;
    const unsigned groups = ((unsigned)w + 63 + kG - 1) / kG;   // w + 63 steps per block
    const unsigned round = groups > (unsigned)(kWaves * kLag) ? groups : (unsigned)(kWaves * kLag);
    const unsigned total = ((blocks - 1) / kWaves) * round + ((blocks - 1) % kWaves) * kLag + groups;

    bool bad = false, rowok = false, stores = false;
    unsigned ft = 0;
    uint8_t *px = raw;
    unsigned prev[kWords], above_left[kWords];
    unsigned next[kG * BPP / 4];
    for (unsigned s = 0; s < total; s++) {
        // block b = r * kWaves + wave takes the super-steps from r * round + wave * kLag on
        const unsigned late = (unsigned)(wave * kLag);
        const unsigned r = s >= late ? (s - late) / round : 0u;
        const int loc = s >= late ? (int)(s - late - r * round) : -1;   // this wave's group in its block
        const unsigned b = r * kWaves + (unsigned)wave;
        if (b < blocks && loc >= 0 && loc < (int)groups) {    // the same for all lanes of a wave
            if (loc == 0) {
                const long long y = (long long)b * kRows + lane - 1;
                rowok = y >= 0 && y < h;
                stores = rowok && lane > 0;
                uint8_t *row = raw + (size_t)(rowok ? y : 0) * rowlen;
                px = row + 1;
                ft = stores ? row[0] : 0u;
                if (ft > 4u) {
                    bad = true;
                    ft = 0;
                }
#pragma unroll
                for (int q = 0; q < kWords; q++)
                    prev[q] = above_left[q] = 0;
                load_group<BPP, kG>(px, rowok, -lane, w, next);
            }
            unsigned cur[kG * BPP / 4], out[kG * BPP / 4];
#pragma unroll
            for (int k = 0; k < kG * BPP / 4; k++) {
                cur[k] = next[k];
                out[k] = 0;
            }
            const int x0 = loc * kG - lane;
            if (loc + 1 < (int)groups)
                load_group<BPP, kG>(px, rowok, x0 + kG, w, next);
#pragma unroll
            for (int j = 0; j < kG; j++) {
                const int x = x0 + j;
                const bool on = rowok && x >= 0 && x < w;
                unsigned up[kWords], res[kWords];
#pragma unroll
                for (int q = 0; q < kWords; q++) {
                    up[q] = from_lane_above(prev[q]);
                    res[q] = 0;
                }
#pragma unroll
                for (int i = 0; i < BPP; i++) {
                    const int sh = 8 * (i & 3);
                    const int a = (int)((prev[i >> 2] >> sh) & 255u);
                    const int bb = (int)((up[i >> 2] >> sh) & 255u);
                    const int c = (int)((above_left[i >> 2] >> sh) & 255u);
                    const int pa = abs(bb - c), pb = abs(a - c), pc = abs(a + bb - 2 * c);
                    const int paeth = (pa <= pb && pa <= pc) ? a : (pb <= pc ? bb : c);
                    const int pred = ft == 1u ? a
                                     : ft == 2u ? bb
                                     : ft == 3u ? (a + bb) >> 1
                                     : ft == 4u ? paeth : 0;
                    const unsigned f = (cur[(j * BPP + i) >> 2] >> (8 * ((j * BPP + i) & 3))) & 255u;
                    const unsigned v = on ? (f + (unsigned)pred) & 255u : 0u;
                    res[i >> 2] |= v << sh;
                    out[(j * BPP + i) >> 2] |= v << (8 * ((j * BPP + i) & 3));
                }
#pragma unroll
                for (int q = 0; q < kWords; q++) {
                    above_left[q] = up[q];
                    prev[q] = res[q];
                }
            }
            store_group<BPP, kG>(px, stores, x0, w, out);
        }
        __syncthreads();   // ... and the stores of this super-step are visible to the workgroup
    }
    return bad;
}

__global__ __launch_bounds__(kUnfilterThreads) void png_unfilter_kernel(
    uint8_t *raw, const DecImage *__restrict__ table, unsigned *__restrict__ flagwords)
{
    __shared__ unsigned sh_bad;
    const DecImage im = table[blockIdx.x];
    if (threadIdx.x == 0)
        sh_bad = 0;
    __syncthreads();
    uint8_t *base = raw + im.raw0;
    bool bad;
    switch (im.bpp) {
    case 1: bad = unfilter_image<1>(base, (int)im.h, (int)im.w, im.rowlen); break;
    case 2: bad = unfilter_image<2>(base, (int)im.h, (int)im.w, im.rowlen); break;
    case 3: bad = unfilter_image<3>(base, (int)im.h, (int)im.w, im.rowlen); break;
    case 4: bad = unfilter_image<4>(base, (int)im.h, (int)im.w, im.rowlen); break;
    case 6: bad = unfilter_image<6>(base, (int)im.h, (int)im.w, im.rowlen); break;
    default: bad = unfilter_image<8>(base, (int)im.h, (int)im.w, im.rowlen); break;
    }
    if (bad)
        atomicOr(&sh_bad, 1u);
    __syncthreads();
    if (threadIdx.x == 0)
        flagwords[blockIdx.x] = sh_bad ? kFlagBad : 0u;
}

// ---- unpack ---------------------------------------------------------------------------------------

// The image a workgroup of the unpack grid works on: the last one with blk0 <= blockIdx.x.
__device__ __forceinline__ int image_of_block(const DecImage *__restrict__ table, int n)
{
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (table[mid].blk0 <= blockIdx.x)
            lo = mid;
        else
            hi = mid - 1;
    }
    return lo;
}

__global__ __launch_bounds__(kUnpackThreads) void png_unpack_kernel(
    const uint8_t *__restrict__ raw, const DecImage *__restrict__ table, int n,
    const uint8_t *__restrict__ palettes, uint8_t *__restrict__ images,
    unsigned *__restrict__ flagwords)
{
    const int img = image_of_block(table, n);
    const DecImage im = table[img];
    const unsigned npx = im.h * im.w;   // below 2^31
    const unsigned p0 = (blockIdx.x - im.blk0) * (unsigned)kUnpackPx;
    const uint8_t *src = raw + im.raw0;
    const uint8_t *pal = im.ctype == 3 ? palettes + (size_t)img * 768 : nullptr;
    uint8_t *dst = images + im.first * 3;
    const bool rgb = im.ctype == 2 || im.ctype == 6;
    int colour = 0;
    for (int k = 0; k < kUnpackPx / kUnpackThreads; k++) {
        const unsigned p = p0 + (unsigned)k * kUnpackThreads + threadIdx.x;
        if (p >= npx)
            break;
        const unsigned y = p / im.w, x = p - y * im.w;
        const uint8_t *s = src + (size_t)y * im.rowlen + 1 + (size_t)x * im.bpp;
        unsigned r, g, bl;
        r = s[0];
        if (rgb) {
            g = s[im.sample];
            bl = s[2 * im.sample];
        } else if (pal) {
            const uint8_t *e = pal + 3 * r;
            r = e[0];
            g = e[1];
            bl = e[2];
        } else {
            g = bl = r;
        }
        uint8_t *o = dst + (size_t)p * 3;
        o[0] = (uint8_t)bl;
        o[1] = (uint8_t)g;
        o[2] = (uint8_t)r;
        colour |= (r != g || g != bl) ? 1 : 0;
    }
    if (__syncthreads_or(colour) && threadIdx.x == 0)
        atomicOr(&flagwords[img], kFlagColour);
}

__global__ __launch_bounds__(256) void png_flags_kernel(const unsigned *__restrict__ flagwords, int n,
                                                        uint8_t *__restrict__ image_flags)
{
    const int i = (int)(blockIdx.x * 256 + threadIdx.x);
    if (i < n) {
        const unsigned f = flagwords[i];
        image_flags[i] = (uint8_t)(((f & kFlagColour) ? 0u : RF_PNG_FLAG_GREY) |
                                   ((f & kFlagBad) ? RF_PNG_FLAG_BAD_FILTER : 0u));
    }
}

// ---- the plan of a call (host) --------------------------------------------------------------------

inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

struct DecPlan {
    std::vector<DecImage> images;
    unsigned long long pixels;
    unsigned long long blocks;   // workgroups of the unpack grid
};

// Bytes per pixel of a format, 0 for one the library does not read.
int format_bpp(int format, int *ctype, int *sample)
{
    const int depth = format >> 8, ct = format & 255;
    if (format < 0 || (depth != 8 && depth != 16))
        return 0;
    int chans;
    switch (ct) {
    case 0: chans = 1; break;
    case 2: chans = 3; break;
    case 3: chans = depth == 8 ? 1 : 0; break;
    case 4: chans = 2; break;
    case 6: chans = 4; break;
    default: chans = 0;
    }
    *ctype = ct;
    *sample = depth / 8;
    return chans * (depth / 8);
}

int plan_decode(const char *who, int n, const int *heights, const int *widths, const int *formats,
                const unsigned long long *raw_offsets, const void *palettes, DecPlan *plan)
{
    if (n < 0)
        return fail(RF_E_BADARG, "%s: bad size n=%d", who, n);
    if (n > 0 && (!heights || !widths || !formats))
        return fail(RF_E_BADARG, "%s: NULL pointer", who);
    if (!launch_fits((unsigned long long)n, kUnfilterThreads))   // the unfilter kernel: a workgroup per image
        return fail(RF_E_UNSUPPORTED, "%s: too many images for one launch", who);
    plan->images.resize((size_t)n);
    plan->pixels = plan->blocks = 0;
    for (int i = 0; i < n; i++) {
        if (heights[i] <= 0 || widths[i] <= 0)
            return fail(RF_E_BADARG, "%s: bad size of image %d: h=%d w=%d", who, i, heights[i],
                        widths[i]);
        int ctype = 0, sample = 0;
        const int bpp = format_bpp(formats[i], &ctype, &sample);
        if (bpp == 0)
            return fail(RF_E_UNSUPPORTED, "%s: format 0x%x of image %d (depth 8 or 16 with colour "
                                          "type 0, 2, 4, 6; depth 8 with colour type 3)", who,
                        formats[i], i);
        const unsigned long long rowlen = 1 + (unsigned long long)widths[i] * bpp;
        const unsigned long long rawlen = rowlen * (unsigned long long)heights[i];
        const unsigned long long px = (unsigned long long)heights[i] * widths[i];
        if (rawlen >= (1ull << 31) || px >= (1ull << 31))
            return fail(RF_E_UNSUPPORTED, "%s: the raw stream or the pixels of image %d (%dx%d) "
                                          "reach 2^31", who, i, widths[i], heights[i]);
        if (raw_offsets && raw_offsets[i + 1] - raw_offsets[i] != rawlen)
            return fail(RF_E_BADARG, "%s: raw length of image %d is %llu B, its size and format "
                                     "need %llu B", who, i, raw_offsets[i + 1] - raw_offsets[i],
                        rawlen);
        if (raw_offsets && ctype == 3 && !palettes)
            return fail(RF_E_BADARG, "%s: NULL pointer: image %d has a palette", who, i);
        const unsigned long long nblk = (px + kUnpackPx - 1) / kUnpackPx;
        if (!launch_fits(plan->blocks + nblk, kUnpackThreads))
            return fail(RF_E_UNSUPPORTED, "%s: more pixels than one grid takes", who);
        DecImage &im = plan->images[i];
        im.raw0 = raw_offsets ? raw_offsets[i] : 0;
        im.first = plan->pixels;
        im.h = (unsigned)heights[i];
        im.w = (unsigned)widths[i];
        im.rowlen = (unsigned)rowlen;
        im.bpp = (unsigned)bpp;
        im.ctype = (unsigned)ctype;
        im.sample = (unsigned)sample;
        im.blk0 = (unsigned)plan->blocks;
        im.nblk = (unsigned)nblk;
        plan->pixels += px;
        plan->blocks += nblk;
    }
    return RF_OK;
}

// The workspace: [image table][flag words], each part rounded up to 256 bytes.
inline size_t decode_workspace(size_t n) { return align256(sizeof(DecImage) * n) + align256(4 * n); }

}  // namespace
}  // namespace rf

extern "C" size_t rf_png_unfilter_workspace_bytes(int n, const int *heights, const int *widths,
                                                  const int *formats)
{
    rf::DecPlan plan;
    if (n <= 0 || rf::plan_decode("rf_png_unfilter_workspace_bytes", n, heights, widths, formats,
                                  nullptr, nullptr, &plan) != RF_OK)
        return 0;
    return rf::decode_workspace((size_t)n);
}

extern "C" int rf_png_unfilter_ragged_u8(uint8_t *raw, const unsigned long long *raw_offsets, int n,
                                         const int *heights, const int *widths, const int *formats,
                                         const uint8_t *palettes, uint8_t *images,
                                         uint8_t *image_flags, void *workspace,
                                         size_t workspace_bytes, void *stream_)
{
    using namespace rf;
    const char *who = "rf_png_unfilter_ragged_u8";
    if (n == 0)
        return RF_OK;
    if (n > 0 && (!raw || !raw_offsets || !heights || !widths || !formats || !images ||
                  !image_flags || !workspace))
        return fail(RF_E_BADARG, "%s: NULL pointer", who);
    DecPlan plan;
    const int rc = plan_decode(who, n, heights, widths, formats, raw_offsets, palettes, &plan);
    if (rc != RF_OK)
        return rc;
    const size_t need = decode_workspace((size_t)n);
    if (workspace_bytes < need)
        return fail(RF_E_WORKSPACE, "%s: workspace %zu B < %zu B", who, workspace_bytes, need);
    if ((uintptr_t)workspace % 16 != 0)
        return fail(RF_E_BADARG, "%s: the workspace must be 16-byte aligned", who);
    if (ranges_overlap(images, (size_t)plan.pixels * 3, raw + raw_offsets[0],
                       (size_t)(raw_offsets[n] - raw_offsets[0])))
        return fail(RF_E_BADARG, "%s: images overlap raw", who);
    hipStream_t stream = (hipStream_t)stream_;
    if (stream_is_capturing(stream))
        return fail(RF_E_UNSUPPORTED, "%s: synchronises its stream and cannot be captured into a "
                                      "graph", who);
    // the host table must outlive the copy: the copy is waited for before the launches (this is
    // the call's one synchronisation of `stream`)
    RF_HIP_CHECK(hipMemcpyAsync(workspace, plan.images.data(), sizeof(DecImage) * (size_t)n,
                                hipMemcpyHostToDevice, stream));
    RF_HIP_CHECK(hipStreamSynchronize(stream));
    char *wsb = static_cast<char *>(workspace);
    const DecImage *table = reinterpret_cast<const DecImage *>(wsb);
    unsigned *flagwords = reinterpret_cast<unsigned *>(wsb + align256(sizeof(DecImage) * (size_t)n));
    hipLaunchKernelGGL(png_unfilter_kernel, dim3((unsigned)n), dim3(kUnfilterThreads), 0, stream, raw,
                       table, flagwords);
    hipLaunchKernelGGL(png_unpack_kernel, dim3((unsigned)plan.blocks), dim3(kUnpackThreads), 0, stream,
                       raw, table, n, palettes, images, flagwords);
    hipLaunchKernelGGL(png_flags_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream,
                       flagwords, n, image_flags);
    RF_HIP_CHECK(hipGetLastError());
    return RF_OK;
}
