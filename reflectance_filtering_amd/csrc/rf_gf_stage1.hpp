// rf_gf_stage1.hpp -- stage 1 of the 8-bit guided filter (rf_gf.hip, the only unit that includes this):
// exact box sums of the guide / src quantities with the per-pixel algebra fused behind them
// (gf_stage1_kernel), the grey probe and the plane interleave of 3-channel sources, and what stage 1
// leaves for the exact-row stage 2 (GfExactOut).  The arithmetic contract is in rf_gf.hip's header.
#pragma once
#include "rf_gf_algebra.hpp"

namespace rf {
namespace {

// ------------------------------------------------------------------------------------------
// stage 1 + per-pixel algebra
// ------------------------------------------------------------------------------------------
// Threads per workgroup and columns per thread (strip width incl. halo = threads x columns) by
// the number of src channels computed.  One channel (13 quantities): 256 x 3 - 40 KB of prefix
// sums, 4 workgroups = 16 waves per CU, 768-column strips (2r of them halo).  Three channels
// (21 quantities): 256 x 2 - 43 KB, 3 workgroups = 12 waves per CU.  Measured alternatives for
// three channels (8 x 4K pass, best rows per segment each): 320 x 2 (15 waves per CU, seven
// strips cover 3840 columns exactly, but five waves per workgroup load the four SIMDs unevenly
// between barriers) 5.04 ms against 4.95; 512 x 1 at 80 registers (24 waves per CU, a fifth
// more scan work per pixel) 5.56 ms.
// Grey guide (RF_GF_GREY_AS_BGR, QuantGrey): 2 + 2 x SCN quantities, so the prefix sums would leave
// room for wider strips.  Measured (8 x 4K, radius 52 / 45): one src channel 3 / 6 / 8 columns per
// thread 1.35 / 1.39 / 1.45 ms per pass, three src channels 3 / 4 mixed (+2 % / -7 %): the scan work
// wide strips save does not pay for fewer, longer workgroups - 256 x 3 (profiles/r07_gf_grey_guide.md).
// (-DRF_GF_GREY_S1_COLS1 / -DRF_GF_GREY_S1_COLS3: other widths for such A/B builds)
#ifndef RF_GF_GREY_S1_COLS1
#define RF_GF_GREY_S1_COLS1 3
#endif
#ifndef RF_GF_GREY_S1_COLS3
#define RF_GF_GREY_S1_COLS3 3
#endif
constexpr int stage1_threads(int, bool = false) { return 256; }
constexpr int stage1_cols(int scn, bool grey = false)
{
    return grey ? (scn == 1 ? RF_GF_GREY_S1_COLS1 : RF_GF_GREY_S1_COLS3) : (scn == 1 ? 3 : 2);
}
constexpr int stage1_nq(int scn, bool grey) { return grey ? 2 + 2 * scn : 9 + 4 * scn; }

// Grey guide (RF_GF_GREY_AS_BGR): one guide byte I per pixel stands for three equal channels
// I_0 = I_1 = I_2 = I.  Of the quantities of Quant<SCN> only I, I*I, p_s and p_s*I are distinct, the
// rest are copies: q: 0 I | 1 I*I | 2.. p_s | then p_s*I.  Their window sums are the integers the
// 9 + 4*SCN sums of the replicated guide hold, so their means are the same floats; expand() lays
// them out in the order of Quant<SCN> and the unchanged algebra runs on that - the same float
// operations on the same operands, including the small-eps determinant branch, which a grey guide
// takes often (det = eps^2 (3 var + eps)).
template <int SCN>
struct QuantGrey {
    static constexpr int NQ = 2 + 2 * SCN;
    static constexpr int NFULL = 9 + 4 * SCN;  // entries of the expanded mean vector
    template <bool NEG>
    __device__ static inline void accumulate(int g, const int *p, uint32_t *acc)
    {
        const int sg = NEG ? -g : g;
        acc[0] += (uint32_t)sg;
        acc[1] += (uint32_t)(sg * g);
#pragma unroll
        for (int s = 0; s < SCN; s++) {
            const int ps = NEG ? -p[s] : p[s];
            acc[2 + s] += (uint32_t)ps;
            acc[2 + SCN + s] += (uint32_t)(ps * g);
        }
    }
    __device__ static inline void expand(const float *m, float *full)
    {
#pragma unroll
        for (int g = 0; g < 3; g++)
            full[g] = m[0];
#pragma unroll
        for (int e = 3; e < 9; e++)
            full[e] = m[1];
#pragma unroll
        for (int s = 0; s < SCN; s++) {
            full[9 + s] = m[2 + s];
#pragma unroll
            for (int g = 0; g < 3; g++)
                full[9 + SCN + 3 * s + g] = m[2 + SCN + s];
        }
    }
};

// Inclusive prefix sum over the 64 lanes of a wave with DPP moves (4 shifts inside each row of
// 16 lanes, then the row totals are broadcast forward): 6 VALU instructions instead of the 6
// ds_bpermute round trips of a __shfl_up scan.
__device__ inline uint32_t wave_inclusive_scan(uint32_t v)
{
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, true);  // row_shr:1
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, true);  // row_shr:2
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, true);  // row_shr:4
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, true);  // row_shr:8
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false); // row_bcast:15
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false); // row_bcast:31
    return v;
}

// mean = (float)((double)S * scale), OpenCV's `(float)(sum * scale)` on the exact window sum S.
// (double)S is formed without a conversion instruction: 2^52 + S has the bit pattern
// {0x43300000, S}, and fma(2^52 + S, scale, -(2^52 * scale)) rounds the exact product S * scale
// once (2^52 * scale is a power-of-two multiple of scale, hence exact) - the same double as
// cvt + mul, one 4-cycle instruction less per quantity and pixel.  nbias = -(2^52 * scale).
__device__ inline float mean_of(uint32_t s, double scale, double nbias)
{
    return (float)__fma_rn(__hiloint2double(0x43300000, (int)s), scale, nbias);
}

// colour[img] != 0  <=>  some pixel of the 3-channel image has unequal channels.
// grid: (blocks per image, images); colour[] zeroed beforehand.  compact (optional): [img][npx]
// bytes that receive channel 0 of every pixel - for an image that turns out grey this IS the
// image, one byte per pixel, and what the first pass's stage 1 then reads (see rf_gf_u8).
__global__ __launch_bounds__(256) void gf_grey_probe_kernel(const uint8_t *__restrict__ src,
                                                            int *__restrict__ colour, size_t npx,
                                                            uint8_t *__restrict__ compact)
{
    const uint8_t *simg = src + (size_t)blockIdx.y * npx * 3;
    uint8_t *cimg = compact ? compact + (size_t)blockIdx.y * npx : nullptr;
    const size_t nquads = npx / 4;  // 4 pixels = 12 bytes = 3 dwords (image base is 4-aligned
                                    // only when npx*3*img is; use byte-safe loads)
    bool diff = false;
    for (size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x; q < nquads;
         q += (size_t)gridDim.x * blockDim.x) {
        uint32_t d0, d1, d2;
        __builtin_memcpy(&d0, simg + q * 12, 4);
        __builtin_memcpy(&d1, simg + q * 12 + 4, 4);
        __builtin_memcpy(&d2, simg + q * 12 + 8, 4);
        // bytes: b0 g0 r0 b1 | g1 r1 b2 g2 | r2 b3 g3 r3 ; grey <=> every pixel's 3 bytes equal
        const uint32_t p0 = d0 & 0xffffffu, p1 = (d0 >> 24) | ((d1 & 0xffffu) << 8);
        const uint32_t p2 = (d1 >> 16) | ((d2 & 0xffu) << 16), p3 = d2 >> 8;
        diff |= p0 != (p0 & 0xffu) * 0x010101u || p1 != (p1 & 0xffu) * 0x010101u ||
                p2 != (p2 & 0xffu) * 0x010101u || p3 != (p3 & 0xffu) * 0x010101u;
        if (cimg != nullptr) {
            const uint32_t c4 = (p0 & 0xffu) | ((p1 & 0xffu) << 8) | ((p2 & 0xffu) << 16) | (p3 << 24 & 0xff000000u);
            __builtin_memcpy(cimg + q * 4, &c4, 4);
        }
    }
    if (blockIdx.x == 0 && threadIdx.x < (int)(npx - nquads * 4)) {
        const uint8_t *p = simg + (nquads * 4 + threadIdx.x) * 3;
        diff |= p[0] != p[1] || p[1] != p[2];
        if (cimg != nullptr)
            cimg[nquads * 4 + threadIdx.x] = p[0];
    }
    if (diff)
        colour[blockIdx.y] = 1;
}

// Last pass of a colour image that travelled as planes: planes [img][3][npx] -> dst [img][npx][3].
// grid: (blocks per image, images); images whose flag colour[img] is 0 (grey: their last pass wrote dst
// itself) are skipped.  Four pixels per thread: three 4-byte loads, one 12-byte store.
__global__ __launch_bounds__(256) void gf_interleave3_kernel(const uint8_t *__restrict__ planes,
                                                             uint8_t *__restrict__ dst, size_t npx,
                                                             const int *__restrict__ colour)
{
    if (colour[blockIdx.y] == 0)
        return;
    const uint8_t *p = planes + (size_t)blockIdx.y * npx * 3;
    uint8_t *d = dst + (size_t)blockIdx.y * npx * 3;
    const size_t nquads = npx / 4;
    for (size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x; q < nquads;
         q += (size_t)gridDim.x * blockDim.x) {
        uint32_t c0, c1, c2;
        __builtin_memcpy(&c0, p + q * 4, 4);
        __builtin_memcpy(&c1, p + npx + q * 4, 4);
        __builtin_memcpy(&c2, p + 2 * npx + q * 4, 4);
        // bytes out: b0 g0 r0 b1 | g1 r1 b2 g2 | r2 b3 g3 r3   (channel planes c0, c1, c2)
        const uint32_t o[3] = {
            (c0 & 0xffu) | ((c1 & 0xffu) << 8) | ((c2 & 0xffu) << 16) | ((c0 & 0xff00u) << 16),
            ((c1 >> 8) & 0xffu) | (((c2 >> 8) & 0xffu) << 8) | (((c0 >> 16) & 0xffu) << 16) |
                (((c1 >> 16) & 0xffu) << 24),
            ((c2 >> 16) & 0xffu) | ((c0 >> 24) << 8) | ((c1 >> 24) << 16) | ((c2 >> 24) << 24)};
        __builtin_memcpy(d + q * 12, o, 12);
    }
    if (blockIdx.x == 0 && threadIdx.x < (int)(npx - nquads * 4)) {
        const size_t i = nquads * 4 + threadIdx.x;
        d[i * 3 + 0] = p[i];
        d[i * 3 + 1] = p[npx + i];
        d[i * 3 + 2] = p[2 * npx + i];
    }
}

// grid: (strips, row segments, images).  ab: [img][SPX][h][w][4] float (g<3 alpha, g=3 beta).
// SCN = src channels computed, SPX = src bytes per pixel (SCN, or 3 with SCN = 1 for a grey
// 3-channel image whose first channel stands for all three).
// MODE (iterated calls: the guide is the same in every pass, /root/reference/README.md:66; only
// kS1Full is used unless the experiment switch "gf_guide_cache" is set, see rf_gf_u8):
//   kS1Full    all 9 + 4*SCN quantities, nothing kept
//   kS1Keep    the same, and the guide half of the algebra (mean I_g, inverse covariance: kGsFloats
//              floats per pixel) is stored to gs                         - first pass
//   kS1Reuse   only the 4*SCN src quantities are box-summed; the guide half is read from gs
//              (requested at the top of a row, used at its end)          - later passes
enum { kS1Full = 0, kS1Keep = 1, kS1Reuse = 2 };

// "Exact rows" (rf_gf_fused.hpp): what stage 1 leaves for a stage 2 without a row walk.
//   xf    [img * groups + group][row][plane 0..3][nb]  double: the sum of the plane's 16 values of
//         image columns 16 b .. 16 b + 15 of that row (nb = w / 16), formed as a butterfly over the 16
//         lanes that hold them (ds_swizzle: the LDS crossbar, no LDS memory).  In a row that passes
//         the exactness test every partial sum is exact, so the order is immaterial; in a row that
//         does not, nobody reads them.
//   xstat [img * groups + group][row][strip * 8 + wave * 2 + half]  two packed words per half-wave:
//         {alpha_0..2 jointly, beta}, each (top 16 bits of the largest magnitude's bit pattern << 1)
//         << 16 | 0xffff - (top 16 bits of the smallest non-zero magnitude's (bits << 1) - 2).
//         gf_exact_rows_kernel turns a row's words into its exactness flag.
struct GfExactOut {
    double *xf;
    uint2 *xstat;
    int nb, slots;  // 16-column blocks per row; statistic slots per row (strips x 8)
};
template <int PATTERN>
__device__ __forceinline__ double swizzle_add(double d)
{
    const int lo = __builtin_amdgcn_ds_swizzle(__double2loint(d), PATTERN);
    const int hi = __builtin_amdgcn_ds_swizzle(__double2hiint(d), PATTERN);
    return d + __hiloint2double(hi, lo);
}
template <int PATTERN>
__device__ __forceinline__ uint32_t swizzle_pkmax(uint32_t v)
{
    typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
    const uint32_t o = (uint32_t)__builtin_amdgcn_ds_swizzle((int)v, PATTERN);
    u16x2 a, b;
    __builtin_memcpy(&a, &v, 4);
    __builtin_memcpy(&b, &o, 4);
    const u16x2 m = __builtin_elementwise_max(a, b);
    uint32_t r;
    __builtin_memcpy(&r, &m, 4);
    return r;
}
// ds_swizzle bit-mask mode: lane' = ((lane & and) | or) ^ xor within 32 lanes
constexpr int swz_xor(int x) { return (x << 10) | 0x1f; }
// Diagnostic build only (-DRF_GF_S1_STAMP, tools/gf_s1_stamp.py): shader cycles per phase of the row
// loop, summed over waves, in a buffer of their own; no output depends on them.
#ifdef RF_GF_S1_STAMP
__device__ unsigned long long g_s1_stamps[16];
#define RF_S1_STAMP(i)                                                  \
    do {                                                                \
        const unsigned long long now_ = __builtin_amdgcn_s_memtime();   \
        st_acc[i] += now_ - st_t;                                       \
        st_t = now_;                                                    \
    } while (0)
#else
#define RF_S1_STAMP(i) do { } while (0)
#endif
// (waves per SIMD: the one-channel kernel is built for four - 128 registers -, which the exact-row
//  additions would otherwise miss by one register; the three-channel kernel for three)
// GREY: the guide is one byte per pixel standing for three equal channels (QuantGrey; plain stage 1
// only, MODE = kS1Full and no exact rows).
// RAGGED (rf_gf_ragged_u8; one src channel, plain stage 1): a 1-D grid of items (image, strip, segment)
// from rag.items; h, w, seg_rows and the image's first pixel come from its record in rag.img.  The
// strip geometry (hl, out_w) depends on the radius alone and stays launch-wide.
template <int SCN, int SPX, int MODE, bool EXACT = false, bool GREY = false, bool RAGGED = false>
__global__ __launch_bounds__(stage1_threads(SCN, GREY))
    __attribute__((amdgpu_waves_per_eu(SCN == 1 ? 4 : 3))) void gf_stage1_kernel(
    const uint8_t *__restrict__ guide, const uint8_t *__restrict__ src, float *__restrict__ ab,
    int h, int w, int radius, float eps_f, int eps_small, int seg_rows,
    const int *__restrict__ colour, float *__restrict__ gs, int ab_groups, int hl, int out_w,
    const GfExactOut xo, const uint8_t *__restrict__ src_planar, const GfRagged rag)
{
    static_assert(!RAGGED || (SCN == 1 && SPX == 1 && MODE == kS1Full && !EXACT),
                  "ragged lists: one src channel, plain stage 1");
    // src_planar (three-channel kernel, later passes of an iterated call): the src channels as three
    // planes [img][3][h][w] - what the previous pass's column walk left - instead of interleaved
    static_assert(!EXACT || MODE == kS1Full, "exact rows: plain stage 1 only");
    static_assert(!GREY || (MODE == kS1Full && !EXACT), "grey guide: plain stage 1 only");
    // hl, out_w: the strip's geometry - its kACW columns are image columns xs - hl .. xs - hl + kACW - 1
    // (xs = strip index x out_w), of which columns hl .. hl + out_w - 1 are its outputs; hl >= radius
    // and kACW - hl - out_w >= radius (rf_gf_u8 picks them, see gf_strip_geometry)
    // ab_groups: plane groups (src channels) an image has in ab - SPX, or 3 when a grey 3-channel
    // image is read from its one-byte-per-pixel intermediate (SPX = 1, see rf_gf_u8)
    // the workgroup's strip, segment and image; pix0 = first pixel of its image
    int bx = blockIdx.x, by = blockIdx.y, bz = blockIdx.z;
    size_t pix0;
    if constexpr (RAGGED) {
        const GfRagItem it = rag.items[blockIdx.x];
        const GfRagImg *ri = rag.img + it.img;
        h = ri->h;
        w = ri->w;
        seg_rows = ri->seg_rows;
        bx = it.a;
        by = it.b;
        bz = it.img;
        pix0 = (size_t)ri->px0;
    } else {
        pix0 = (size_t)blockIdx.z * ((size_t)h * w);
    }
    if (wrong_variant<SCN>(colour, bz))
        return;
    using Q = std::conditional_t<GREY, QuantGrey<SCN>, Quant<SCN, MODE != kS1Reuse>>;
    constexpr int NQ = Q::NQ;
    constexpr int kGCN = GREY ? 1 : 3;  // guide bytes per pixel
    constexpr int kAThreads = stage1_threads(SCN, GREY), kAWaves = kAThreads / 64;
    constexpr int kACols = stage1_cols(SCN, GREY);
    constexpr int kACW = kAThreads * kACols;
    __shared__ uint32_t pfx[NQ][kACW + 1];
    __shared__ uint32_t wave_acc[NQ][kAWaves];

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int xs = bx * out_w;
    const int ys = by * seg_rows;
    const int ye = min(ys + seg_rows, h);
    const size_t npx = (size_t)h * w;
    const uint8_t *gimg = guide + pix0 * kGCN;
    const uint8_t *simg = src + pix0 * SPX;
    float *abimg = ab + pix0 * (ab_groups * 4);
    float *gsimg = MODE == kS1Full ? nullptr : gs + pix0 * kGsFloats;
    const int ks = 2 * radius + 1;
    const double scale = 1.0 / (double)(ks * ks);
    const double nbias = -(4503599627370496.0 * scale);

    // byte offsets of the thread's columns within an image row (guide: kGCN bytes per pixel, src: SPX);
    // a row's bytes are then (wave-uniform row pointer) + (32-bit lane offset): no 64-bit vector
    // arithmetic per load
    const bool planar = SCN == 3 && src_planar != nullptr;
    const uint8_t *pimg = planar ? src_planar + pix0 * 3 : nullptr;
    uint32_t gx3[kACols], gxs[kACols];
#pragma unroll
    for (int k = 0; k < kACols; k++) {
        const int gx = border_interpolate(xs - hl + tid * kACols + k, w, RF_BORDER_REFLECT);
        gx3[k] = (uint32_t)gx * (uint32_t)kGCN;
        gxs[k] = planar ? (uint32_t)gx : (uint32_t)gx * (uint32_t)SPX;
    }

    uint32_t V[kACols][NQ];
#pragma unroll
    for (int k = 0; k < kACols; k++)
#pragma unroll
        for (int q = 0; q < NQ; q++)
            V[k][q] = 0;

    // (Byte loads, 3 x (3 + SCN) per row step and thread, are not what limits this kernel: fetching
    // a thread's three pixels as one 12-byte load and picking the bytes apart was measured 10 %
    // SLOWER - the extra VALU work costs more than the vector-memory instructions it saves.)
    // One image row of the strip enters (or leaves) the vertical running sums.  The row's bytes are
    // read through a buffer descriptor over that row (wave-uniform base: scalar arithmetic only)
    // with the lane's constant 32-bit byte offset: no vector address arithmetic per load.
    auto add_row = [&](int yy, auto neg_c) __attribute__((always_inline)) {
        constexpr bool NEG = decltype(neg_c)::value;
        const int gy = border_interpolate(yy, h, RF_BORDER_REFLECT);
        const auto rg = __builtin_amdgcn_make_buffer_rsrc(
            const_cast<uint8_t *>(gimg + (size_t)gy * w * kGCN), 0, w * kGCN, 0x00020000);
        // (planar: one descriptor over the three planes' common row offset .. the last plane's row,
        //  channel sc at byte sc * npx + column; interleaved: the row's w * SPX bytes)
        const auto rp = __builtin_amdgcn_make_buffer_rsrc(
            const_cast<uint8_t *>(planar ? pimg + (size_t)gy * w : simg + (size_t)gy * w * SPX), 0,
            planar ? (int)(2 * npx) + w : w * SPX, 0x00020000);
        const int pstep = planar ? (int)npx : 1;
#pragma unroll
        for (int k = 0; k < kACols; k++) {
            int p[SCN];
            if constexpr (GREY) {
                const int g = __builtin_amdgcn_raw_buffer_load_b8(rg, (int)gx3[k], 0, 0);
#pragma unroll
                for (int sc = 0; sc < SCN; sc++)
                    p[sc] = __builtin_amdgcn_raw_buffer_load_b8(rp, (int)gxs[k], sc * pstep, 0);
                Q::template accumulate<NEG>(g, p, V[k]);
            } else {
                const uint32_t g01 = __builtin_amdgcn_raw_buffer_load_b16(rg, (int)gx3[k], 0, 0);
                const int g2 = __builtin_amdgcn_raw_buffer_load_b8(rg, (int)gx3[k] + 2, 0, 0);
#pragma unroll
                for (int sc = 0; sc < SCN; sc++)
                    p[sc] = __builtin_amdgcn_raw_buffer_load_b8(rp, (int)gxs[k], sc * pstep, 0);
                Q::template accumulate<NEG>((int)(g01 & 0xffu), (int)(g01 >> 8), g2, p, V[k]);
            }
        }
    };
    using RowIn = std::integral_constant<bool, false>;
    using RowOut = std::integral_constant<bool, true>;

    for (int yy = ys - radius; yy < ys + radius; yy++)
        add_row(yy, RowIn{});
    if (tid == 0)
#pragma unroll
        for (int q = 0; q < NQ; q++)
            pfx[q][0] = 0;

    // wave_acc[q][j] accumulates, over all rows so far, the totals of the waves to the left of
    // wave j (uint32 wrap-around is exact): a wave adds its total to the entries of the waves to
    // its right with one LDS atomic per quantity, and every thread gets its row's base as the
    // difference between the entry now and one row ago - one broadcast read and one subtraction
    // per quantity instead of kAWaves - 1 reads, selects and adds
    uint32_t acc_prev[NQ];
#pragma unroll
    for (int q = 0; q < NQ; q++)
        acc_prev[q] = 0;
    if (tid < kAWaves)
#pragma unroll
        for (int q = 0; q < NQ; q++)
            wave_acc[q][tid] = 0;
    __syncthreads();

    // Per-pixel phase (window means -> algebra -> alpha/beta): the strip's columns are dealt to the
    // threads one by one, thread t taking columns pc[k] = t' + kAThreads * k (the prefix sums are in LDS:
    // any thread can serve any column).  A wave then stores 64 consecutive pixels (1 KB) per
    // instruction, its 16-lane rows are 16 consecutive columns, and with a halo of a whole wave on
    // either side (hl = 64, out_w = kACW - 128: 3840 = 6 x 640, 1920 = 3 x 640) two of the strip's
    // twelve wave-iterations have no output column at all and are skipped - which waves those are
    // alternates with the workgroup's parity (t' = t rotated by two waves), so that the four SIMDs
    // of a CU see the same load.
    const int tidp = (tid + ((bx + by + bz) & 1) * (kAThreads / 2)) & (kAThreads - 1);
    bool col_ok[kACols];
#pragma unroll
    for (int k = 0; k < kACols; k++) {
        const int c = tidp + kAThreads * k;
        col_ok[k] = c >= hl && c < hl + out_w && xs - hl + c < w;
    }
#ifdef RF_GF_S1_STAMP
    unsigned long long st_acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    unsigned long long st_t = __builtin_amdgcn_s_memtime();
    unsigned long long st_n = 0;
#endif
    for (int y = ys; y < ye; y++) {
        // later passes: the guide records of the row's pixels, used after the barriers
        // (gs: [img][row][kGsFloats][w] - the floats of a record are w apart, so the lanes of a wave
        //  read and write runs of consecutive floats; interleaved 36-byte records made every load
        //  and store instruction of a wave touch 54 cache lines and cost more than they saved)
        float gsr[kACols][kGsFloats];
        if (MODE == kS1Reuse) {
            const float *rec = gsimg + (size_t)y * kGsFloats * w + (xs - hl + tidp);
#pragma unroll
            for (int k = 0; k < kACols; k++) {
                if (!col_ok[k])
                    continue;
#pragma unroll
                for (int e = 0; e < kGsFloats; e++)
                    gsr[k][e] = rec[(size_t)e * w + kAThreads * k];
            }
        }
        add_row(y + radius, RowIn{});
        RF_S1_STAMP(0);
        // inclusive prefix over the strip's columns, per quantity.  The six DPP steps of the wave
        // scan run stage by stage across the quantities: back to back on one quantity every step
        // waits out the VALU-write -> DPP-read hazard (an s_nop per step and quantity)
        uint32_t incl[NQ];
#pragma unroll
        for (int q = 0; q < NQ; q++) {
            uint32_t tsum = V[0][q];
#pragma unroll
            for (int k = 1; k < kACols; k++)
                tsum += V[k][q];
            incl[q] = tsum;
        }
#define RF_SCAN_STAGE(CTRL, ROWMASK, BOUND)                                                  \
    _Pragma("unroll") for (int q = 0; q < NQ; q++) incl[q] +=                                \
        (uint32_t)__builtin_amdgcn_update_dpp(0, (int)incl[q], CTRL, ROWMASK, 0xf, BOUND);
        RF_SCAN_STAGE(0x111, 0xf, true)   // row_shr:1
        RF_SCAN_STAGE(0x112, 0xf, true)   // row_shr:2
        RF_SCAN_STAGE(0x114, 0xf, true)   // row_shr:4
        RF_SCAN_STAGE(0x118, 0xf, true)   // row_shr:8
        RF_SCAN_STAGE(0x142, 0xa, false)  // row_bcast:15
#undef RF_SCAN_STAGE
        // last step (row_bcast:31 into rows 2 and 3) spelled out: hipcc does not fold this one into
        // the add and emits v_mov 0 / v_mov_dpp / v_add per quantity.  Each statement reads a
        // register written NQ instructions earlier, so the DPP read hazard is covered.
        asm volatile("s_nop 1");  // ... whatever hipcc put last before the first statement
#pragma unroll
        for (int q = 0; q < NQ; q++)
            asm volatile("v_add_u32_dpp %0, %0, %0 row_bcast:31 row_mask:0xc bank_mask:0xf"
                         : "+v"(incl[q]));
        RF_S1_STAMP(7);
        {
            // lanes 0 .. kAWaves-2-wave add the wave total (lane 63's prefix) to the entries of the
            // waves to the right
            // (all the totals first, then ONE masked region with the atomics: per quantity hipcc
            //  opens and closes the mask around each)
            const int dstw = wave + 1 + lane;
            uint32_t tot[NQ];
#pragma unroll
            for (int q = 0; q < NQ; q++)
                tot[q] = (uint32_t)__builtin_amdgcn_readlane((int)incl[q], 63);
            if (dstw < kAWaves) {
#pragma unroll
                for (int q = 0; q < NQ; q++)
                    atomicAdd(&wave_acc[q][dstw], tot[q]);
            }
        }
        RF_S1_STAMP(1);
        __syncthreads();
        RF_S1_STAMP(2);
#pragma unroll
        for (int q = 0; q < NQ; q++) {
            const uint32_t acc = wave_acc[q][wave];
            const uint32_t base = acc - acc_prev[q];
            acc_prev[q] = acc;
            uint32_t pk = incl[q] + base;  // inclusive prefix at the thread's last column
#pragma unroll
            for (int k = kACols - 1; k >= 0; k--) {
                pfx[q][tid * kACols + k + 1] = pk;
                pk -= V[k][q];
            }
        }
        RF_S1_STAMP(3);
        __syncthreads();
        RF_S1_STAMP(4);
        // exact rows: largest magnitude (its bit pattern: an infinity or a NaN then counts as the largest
        // exponent there is and fails the row) and smallest non-zero magnitude (as (bits << 1) - 2, which
        // sends a zero to the top) of the row's alpha planes jointly and of its beta plane, per src
        // channel, over this lane's columns
        uint32_t xmx_a[SCN], xmx_b[SCN];
        uint32_t xmn_a[SCN], xmn_b[SCN];
        if (EXACT) {
#pragma unroll
            for (int sc = 0; sc < SCN; sc++) {
                xmx_a[sc] = xmx_b[sc] = 0u;
                xmn_a[sc] = xmn_b[sc] = 0xffffffffu;
            }
        }
#pragma unroll
        for (int k = 0; k < kACols; k++) {
            const int c = tidp + kAThreads * k;
            const int x = xs - hl + c;
            if (!col_ok[k])
                continue;
            float m[NQ];
#pragma unroll
            for (int q = 0; q < NQ; q++)
                m[q] = mean_of(pfx[q][c + radius + 1] - pfx[q][c - radius], scale, nbias);
            float ab_px[4 * SCN];
            if constexpr (GREY) {
                float mf[QuantGrey<SCN>::NFULL];
                QuantGrey<SCN>::expand(m, mf);
                float gsn[kGsFloats];
                gf_guide_algebra(mf, eps_f, eps_small, gsn);
                gf_src_algebra<SCN>(gsn, mf + 9, ab_px);
            } else if (MODE == kS1Reuse) {
                gf_src_algebra<SCN>(gsr[k], m, ab_px);
            } else {
                float gsn[kGsFloats];
                gf_guide_algebra(m, eps_f, eps_small, gsn);
                gf_src_algebra<SCN>(gsn, m + 9, ab_px);
                if (MODE == kS1Keep) {
                    float *rec = gsimg + (size_t)y * kGsFloats * w + x;
#pragma unroll
                    for (int e = 0; e < kGsFloats; e++)
                        rec[(size_t)e * w] = gsn[e];
                }
            }
            // the four planes of a src channel (alpha_0..2, beta) interleaved per pixel: one
            // 16-byte store, and stage 2 reads 256-byte runs per image row instead of 64-byte ones
            // (through a descriptor over the image row: wave-uniform base, the lane's constant offset)
#pragma unroll
            for (int sc = 0; sc < SCN; sc++) {
                const auto rab = __builtin_amdgcn_make_buffer_rsrc(
                    abimg + ((size_t)sc * npx + (size_t)y * w) * 4, 0, w * 16, 0x00020000);
                typedef unsigned u32x4_t __attribute__((ext_vector_type(4)));
                const u32x4_t o = {__float_as_uint(ab_px[4 * sc]), __float_as_uint(ab_px[4 * sc + 1]),
                                   __float_as_uint(ab_px[4 * sc + 2]), __float_as_uint(ab_px[4 * sc + 3])};
                __builtin_amdgcn_raw_buffer_store_b128(o, rab, x * 16, 0, 0);
            }
            if (EXACT) {
                // (col_ok is uniform over a 16-lane row here: hl, out_w and w are multiples of 16)
#pragma unroll
                for (int sc = 0; sc < SCN; sc++) {
                    const float a0 = ab_px[4 * sc], a1 = ab_px[4 * sc + 1], a2 = ab_px[4 * sc + 2],
                                bt = ab_px[4 * sc + 3];
                    xmx_a[sc] = max(max(xmx_a[sc], __float_as_uint(a0) & 0x7fffffffu),
                                    max(__float_as_uint(a1) & 0x7fffffffu, __float_as_uint(a2) & 0x7fffffffu));
                    xmx_b[sc] = max(xmx_b[sc], __float_as_uint(bt) & 0x7fffffffu);
                    xmn_a[sc] = min(min(xmn_a[sc], (__float_as_uint(a0) << 1) - 2u),
                                    min((__float_as_uint(a1) << 1) - 2u, (__float_as_uint(a2) << 1) - 2u));
                    xmn_b[sc] = min(xmn_b[sc], (__float_as_uint(bt) << 1) - 2u);
                    double d[4];
#pragma unroll
                    for (int p = 0; p < 4; p++) {
                        d[p] = (double)ab_px[4 * sc + p];
                        d[p] = swizzle_add<swz_xor(1)>(d[p]);
                        d[p] = swizzle_add<swz_xor(2)>(d[p]);
                        d[p] = swizzle_add<swz_xor(4)>(d[p]);
                        d[p] = swizzle_add<swz_xor(8)>(d[p]);
                    }
                    // lane j < 4 of the 16-lane row stores plane j's sum
                    const double d01 = (lane & 1) ? d[1] : d[0], d23 = (lane & 1) ? d[3] : d[2];
                    const double dsel = (lane & 2) ? d23 : d01;
                    if ((lane & 15) < 4) {
                        double *xr = xo.xf + (((size_t)blockIdx.z * ab_groups + sc) * h + y) * 4 * xo.nb;
                        xr[(lane & 3) * xo.nb + (x >> 4)] = dsel;
                    }
                }
            }
        }
        if (EXACT) {
            // the half-wave's statistics: five butterfly steps over packed 16-bit fields (maximum of
            // the largest, maximum of the inverted smallest), lanes 0 and 32 store
#pragma unroll
            for (int sc = 0; sc < SCN; sc++) {
                uint32_t wa = ((xmx_a[sc] >> 15) << 16) | (0xffffu - (xmn_a[sc] >> 16));
                uint32_t wb = ((xmx_b[sc] >> 15) << 16) | (0xffffu - (xmn_b[sc] >> 16));
                wa = swizzle_pkmax<swz_xor(1)>(wa);
                wb = swizzle_pkmax<swz_xor(1)>(wb);
                wa = swizzle_pkmax<swz_xor(2)>(wa);
                wb = swizzle_pkmax<swz_xor(2)>(wb);
                wa = swizzle_pkmax<swz_xor(4)>(wa);
                wb = swizzle_pkmax<swz_xor(4)>(wb);
                wa = swizzle_pkmax<swz_xor(8)>(wa);
                wb = swizzle_pkmax<swz_xor(8)>(wb);
                wa = swizzle_pkmax<swz_xor(16)>(wa);
                wb = swizzle_pkmax<swz_xor(16)>(wb);
                if ((lane & 31) == 0)
                    xo.xstat[(((size_t)blockIdx.z * ab_groups + sc) * h + y) * xo.slots + blockIdx.x * 8 +
                             wave * 2 + (lane >> 5)] = make_uint2(wa, wb);
            }
        }
        RF_S1_STAMP(5);
        add_row(y - radius, RowOut{});
        RF_S1_STAMP(6);
#ifdef RF_GF_S1_STAMP
        st_n++;
#endif
    }
#ifdef RF_GF_S1_STAMP
    if (lane == 0) {
        for (int i = 0; i < 8; i++)
            atomicAdd(&g_s1_stamps[i], st_acc[i]);
        atomicAdd(&g_s1_stamps[15], st_n);
    }
#endif
}

}  // namespace
}  // namespace rf
