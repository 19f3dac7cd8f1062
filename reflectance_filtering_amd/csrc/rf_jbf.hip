// rf_jbf.hip -- joint bilateral filter, uint8, for gfx950 (MI355X).
//
// Replaces cv2.ximgproc.jointBilateralFilter as called at the reference's
// filter_reflectance.py:60-64.  Arithmetic contract (DESIGN.md "JBF"):
// per output pixel the taps of the radius-r disk are visited row-major, the weight is
// spaceW[k] * colorLUT[L1(joint0, jointTap)] in float32, and sum[c] += weight * src[c] is a
// separately rounded multiply then add -- the order of the 8u path of
// opencv_contrib/modules/ximgproc/src/joint_bilateral_filter.cpp on a non-FMA build.
//
// Kernels (selection in rf_jbf_u8 at the end of the file):
//   jbf_tile64_kernel  default for radius <= 52: one workgroup = 64x64 output tile (32x128,
//                      16x256 or 128x32 for the image's remainder rows / columns), 1024 threads
//                      (4 waves/SIMD), LDS-staged texel tile, LUT at the end of LDS.
//                      Its kRagged instantiation serves rf_jbf_ragged_u8 (images of different sizes
//                      packed one after another): the tile's image, size and origin come from a
//                      32-byte record per workgroup; everything after that read is the same code.
//   jbf_slab_kernel    radius 53..468: the same 64x64 outputs with the disk's tap rows taken in slabs
//                      (row pitch 208 .. 1008; the grey loop; a colour src in one pass of the colour
//                      loop, or one pass per channel of the grey loop where that leaves no slab).
//                      Its kRagged instantiation serves rf_jbf_ragged_u8 at these radii: every image's
//                      64x64 tiles in one launch, from the same 32-byte records.
//   jbf_tiled2_kernel  64 x TH tiles with 8-byte texels and a clamped/full LUT: used when the
//                      LDS out-of-range probe fails, and by the tuning harness.
//   jbf_generic_kernel untiled, any radius, global-memory gathers (fallback + cross-check).
// Elsewhere:
//   rf_jbf_taploops.hpp  the tap loops of the tiled kernels: jbf_tap_loop_grey4_la2 (the default
//                        for grey tiles: hand-interleaved, gathers two column steps ahead; J1 =
//                        single-channel joint whose pre-scaled texels make v_sad_u32 produce the
//                        gather address), jbf_tap_loop_rgb6 (colour tiles), jbf_tap_loop_grey4 (one
//                        step ahead, A/B aid) and jbf_tap_loop (compiler-scheduled; jbf_tiled2_kernel
//                        and the cross-check).
//   rf_jbf_tables.hip    the parameter tables (colour LUT, tap tables) and their cache (get_tables).
//   rf_jbf_common.hpp    the argument rules and per-pixel pieces shared with rf_jbf_points.hip.
//   rf_jbf_f32.hip       the CV_32F filter (rf_jbf_f32): its own kernels, the same tap tables.
#include <algorithm>
#include <atomic>
#include <mutex>
#include <vector>

#include "rf_jbf_common.hpp"
#include "rf_jbf_tables.hpp"
#include "rf_jbf_taploops.hpp"

namespace rf {
namespace {

constexpr int kTileW = 64;
constexpr int kMaxLds = 160 * 1024;
constexpr int kTlw2 = 144;     // tile row pitch in texels of jbf_tiled2_kernel (radius <= 36)
constexpr int kJbfMaxTiledR4 = 468;  // radius (rounded up to 4) the slab kernel's widest row pitch (1008) holds
// private flag bits above the public RF_JBF_* ones: the test / benchmark switches of
// rf_debug_option() as the kernels see them
constexpr int kJbfStageOnly = 0x1000, kJbfCompilerLoop = 0x2000, kJbfTile64Only = 0x4000;
constexpr int kJbfLookahead1 = 0x8000;  // grey asm loop with its gathers one column step ahead (round-4 form)
constexpr int kJbfNoMsad = 0x10000;     // every wave takes the tap loop with the mask (none the masked-SAD form)
constexpr int kJbfVoteOnly = 0x20000;   // jbf_tile64x2_kernel: write the tiles' vote bytes and leave (set by its launcher only)
constexpr int kJbfNoDeadSkip = 0x40000; // jbf_tile64x2_kernel: waves wholly below the image walk the tap loop all the same

// the test / benchmark switches (rf_debug_option) as they travel to the kernels: private flag bits
int jbf_debug_flags()
{
    return (debug_get(kDbgJbfStageOnly) ? kJbfStageOnly : 0) |
           (debug_get(kDbgJbfCompilerLoop) ? kJbfCompilerLoop : 0) |
           (debug_get(kDbgJbfTile64Only) ? kJbfTile64Only : 0) |
           (debug_get(kDbgJbfLookahead1) ? kJbfLookahead1 : 0) |
           (debug_get(kDbgJbfNoMsad) ? kJbfNoMsad : 0) |
           (debug_get(kDbgJbfNoDeadSkip) ? kJbfNoDeadSkip : 0);
}

// Four consecutive pixels (cn interleaved bytes each, any alignment) -> four packed dwords.
__device__ inline void load_packed4(const uint8_t *img, size_t pix, int cn, uint32_t (&out)[4])
{
    const uint8_t *p = img + pix * (cn < 0 ? 1 : cn);
    if (cn == 3) {
        uint32_t d0, d1, d2;  // one (unaligned) 12-byte load
        __builtin_memcpy(&d0, p, 4);
        __builtin_memcpy(&d1, p + 4, 4);
        __builtin_memcpy(&d2, p + 8, 4);
        out[0] = d0 & 0x00ffffffu;
        out[1] = (d0 >> 24) | ((d1 & 0xffffu) << 8);
        out[2] = (d1 >> 16) | ((d2 & 0xffu) << 16);
        out[3] = d2 >> 8;
    } else {
        uint32_t d0;
        __builtin_memcpy(&d0, p, 4);
        const uint32_t rep = cn < 0 ? 0x010101u : 1u;
        out[0] = (d0 & 0xffu) * rep;
        out[1] = ((d0 >> 8) & 0xffu) * rep;
        out[2] = ((d0 >> 16) & 0xffu) * rep;
        out[3] = (d0 >> 24) * rep;
    }
}

// Packed joint/src values of the four tile columns X = 4k .. 4k+3 of one tile row (image row
// gy >= 0 already border-interpolated, or gy < 0 = outside under BORDER_CONSTANT).  Interior
// columns take the 12-byte path, columns that need border handling go pixel by pixel.
__device__ inline void load_tile_quad(const uint8_t *joint, const uint8_t *src, size_t img, int gy,
                                      int x_first, int w, int jcn, int scn, int border,
                                      uint32_t (&jv)[4], uint32_t (&sv)[4])
{
    if (gy < 0) {
#pragma unroll
        for (int u = 0; u < 4; u++)
            jv[u] = sv[u] = 0u;
        return;
    }
    const size_t row = img + (size_t)gy * w;
    if (x_first >= 0 && x_first + 3 < w) {
        load_packed4(joint, row + x_first, jcn, jv);
        load_packed4(src, row + x_first, scn, sv);
        return;
    }
#pragma unroll
    for (int u = 0; u < 4; u++) {
        const int gx = border_interpolate(x_first + u, w, border);
        jv[u] = gx < 0 ? 0u : load_packed(joint, row + gx, jcn);
        sv[u] = gx < 0 ? 0u : load_packed(src, row + gx, scn);
    }
}

// Workgroups are dealt round-robin to the 8 XCDs (blocks b and b+8 share an L2).  This maps the
// launch index to a tile index such that every XCD works through one contiguous range of tiles,
// so the halo a tile shares with its neighbours is served by that XCD's own L2.  Speed only.
__device__ inline int xcd_contiguous_tile(int b, int nblocks)
{
    const int per = nblocks >> 3;
    return b < (per << 3) ? (b & 7) * per + (b >> 3) : b;
}

__device__ inline float finish_value(float sum, float wsum_or_inv, int flags)
{
    return (flags & RF_JBF_TRUE_DIVISION) ? __fdiv_rn(sum, wsum_or_inv) : __fmul_rn(sum, wsum_or_inv);
}

// Stores a lane's 4 horizontally adjacent outputs.  sums[p][c]; NCH_IN = 1 replicates the single
// accumulated channel.  Interior quads of 3-channel images go out as one 12-byte store.
template <int NCH_IN, int SCN>
__device__ inline void store_quad(uint8_t *dst, size_t img, int oy, int ox0, int h, int w,
                                  const float (&sum)[kPix][NCH_IN], const float (&wsum)[kPix],
                                  int flags)
{
    if (oy >= h || ox0 >= w)
        return;
    uint8_t px[kPix][3];
#pragma unroll
    for (int p = 0; p < kPix; p++) {
        const float d = (flags & RF_JBF_TRUE_DIVISION) ? wsum[p] : __fdiv_rn(1.0f, wsum[p]);
#pragma unroll
        for (int c = 0; c < SCN; c++)
            px[p][c] = saturate_u8(finish_value(sum[p][NCH_IN == 1 ? 0 : c], d, flags));
    }
    uint8_t *o = dst + (img + (size_t)oy * w + ox0) * SCN;
    if (SCN == 3 && ox0 + 3 < w) {
        uint32_t d[3];
        d[0] = px[0][0] | (px[0][1] << 8) | (px[0][2] << 16) | ((uint32_t)px[1][0] << 24);
        d[1] = px[1][1] | (px[1][2] << 8) | (px[2][0] << 16) | ((uint32_t)px[2][1] << 24);
        d[2] = px[2][2] | (px[3][0] << 8) | (px[3][1] << 16) | ((uint32_t)px[3][2] << 24);
        __builtin_memcpy(o, d, 12);
    } else if (SCN == 1 && ox0 + 3 < w) {
        const uint32_t d = px[0][0] | (px[1][0] << 8) | (px[2][0] << 16) | ((uint32_t)px[3][0] << 24);
        __builtin_memcpy(o, &d, 4);
    } else {
#pragma unroll
        for (int p = 0; p < kPix; p++)
            if (ox0 + p < w)
#pragma unroll
                for (int c = 0; c < SCN; c++)
                    o[p * SCN + c] = px[p][c];
    }
}

// ------------------------------------------------------------------------------------------
// Untiled fallback: one thread per output pixel, taps gathered from global memory.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void jbf_generic_kernel(
    const uint8_t *__restrict__ joint, const uint8_t *__restrict__ src, uint8_t *__restrict__ dst,
    int h, int w, int jcn, int scn, int border, const float *__restrict__ lut,
    const int *__restrict__ di, const int *__restrict__ dj, const float *__restrict__ sw, int maxk,
    int flags)
{
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= w || y >= h)
        return;
    const size_t img = (size_t)blockIdx.z * h * w;
    const uint32_t j0 = load_packed(joint, img + (size_t)y * w + x, jcn);
    float sum[3] = {0.f, 0.f, 0.f};
    float wsum = 0.f;
    for (int k = 0; k < maxk; k++) {
        const int yy = border_interpolate(y + di[k], h, border);
        const int xx = border_interpolate(x + dj[k], w, border);
        uint32_t jt = 0, st = 0;
        if (yy >= 0 && xx >= 0) {
            const size_t q = img + (size_t)yy * w + xx;
            jt = load_packed(joint, q, jcn);
            st = load_packed(src, q, scn);
        }
        const uint32_t alpha = __builtin_amdgcn_sad_u8(j0, jt, 0u);
        const float wgt = __fmul_rn(sw[k], lut[alpha]);
        sum[0] = __fadd_rn(sum[0], __fmul_rn(wgt, (float)(st & 0xff)));
        if (scn == 3) {
            sum[1] = __fadd_rn(sum[1], __fmul_rn(wgt, (float)((st >> 8) & 0xff)));
            sum[2] = __fadd_rn(sum[2], __fmul_rn(wgt, (float)((st >> 16) & 0xff)));
        }
        wsum = __fadd_rn(wsum, wgt);
    }
    finish_pixel(dst + (img + (size_t)y * w + x) * scn, sum, wsum, scn, flags);
}

// ------------------------------------------------------------------------------------------
// Tiled kernels: the software-pipelined tap loop.
//
// One workgroup stages its output tile plus halo into LDS (border handling happens there, so the
// tap loop is branch-free); each lane owns 4 horizontally adjacent outputs and slides over the tap
// row, so every texel read and its byte->float conversions feed 4 outputs.  In detail:
//   * the tap row is walked in groups of 4 columns starting at a multiple of 4, so the texel
//     address of column (group g, u) is  lane_base + u*(TLW/4) + g : one VALU add per group,
//     immediates for the rest, and the spatial weights of the 4 columns x 4 outputs are a
//     7-float window of the (symmetric) weight row, fetched from LDS as two aligned float4
//     broadcasts per group (no scalar-memory loads inside the loop, so LDS waits stay counted);
//   * a 3-stage pipeline over columns: the texel of column c+2 and the four LUT gathers of
//     column c+1 are in flight while column c is accumulated;
//   * TH rows per tile (16*TH threads): 32 -> 2 waves/SIMD, 48 -> 3 waves/SIMD;
//   * LUTREP replicas of the colour LUT (32 = conflict-free, 16/8 trade conflicts for LDS).
// Columns outside the disk carry zero weight: w = 0 adds +0.0 to non-negative sums, which is
// bit-identical to skipping the tap.
// jbf_tiled2_kernel LDS: [flag][lutrep lut_len*LUTREP f32][sw (r+1)*sw_len f32][tile (TH+2r) x TLW]
// Tile column X <-> image x = tile_x0 - r4 + X, stored at (X&3)*(TLW/4) + (X>>2): the lane that
// owns outputs 4t..4t+3 reads X = 4t + const, i.e. consecutive lanes read consecutive texels
// (conflict-free) although each lane's own outputs are adjacent; TLW % 32 == 16 keeps the two
// 16-lane rows of a 32-lane LDS group on disjoint banks.
// ------------------------------------------------------------------------------------------
// Block-wide AND of a predicate through one word of the caller's dynamic LDS (HIP's
// __syncthreads_and brings 256 bytes of static LDS with it, which the kernels below cannot spare
// and which would move the end of the allocation the LUT is aligned to).  `word` must have been
// set to 1 before an earlier barrier.  Contains a barrier.
__device__ inline int block_all(int pred, volatile int *word)
{
    if (!pred)
        *word = 0;
    __syncthreads();
    return *word;
}

// Two predicates at once: bit 0 / bit 1 of the result are set iff every thread passed pred0 /
// pred1.  `word` must have been set to 3 before an earlier barrier.
__device__ inline int block_all2(int pred0, int pred1, int *word)
{
    const int keep = (pred0 ? 1 : 0) | (pred1 ? 2 : 0);
    if (keep != 3)
        atomicAnd(word, keep);
    __syncthreads();
    return *reinterpret_cast<volatile int *>(word);
}

// LDS byte address of a pointer into the workgroup's LDS (low 32 bits of the generic pointer).
__device__ inline uint32_t lds_addr(const void *p)
{
    return static_cast<uint32_t>(reinterpret_cast<uintptr_t>(p));
}

template <int SCN, int TH, int LUTREP, bool CLAMP>
__global__ __launch_bounds__(16 * TH) void jbf_tiled2_kernel(
    const uint8_t *__restrict__ joint, const uint8_t *__restrict__ src, uint8_t *__restrict__ dst,
    int h, int w, int jcn, int radius, int border, const float *__restrict__ lut, int lut_len,
    const int *__restrict__ hwtab, const float *__restrict__ swsym, int sw_len, int tiles_x,
    int tiles_per_img, int flags)
{
    constexpr int NT = 16 * TH;
    constexpr int TLW = kTlw2;
    constexpr int Q4 = TLW / 4;
    extern __shared__ __align__(16) unsigned char smem[];
    volatile int *flag_word = reinterpret_cast<volatile int *>(smem);
    float *lutrep = reinterpret_cast<float *>(smem + 16);
    const int lut_bytes = (lut_len * LUTREP * 4 + 15) & ~15;
    float *swl = reinterpret_cast<float *>(smem + 16 + lut_bytes);
    const int sw_bytes = ((radius + 1) * sw_len * 4 + 15) & ~15;
    uint2 *tile = reinterpret_cast<uint2 *>(smem + 16 + lut_bytes + sw_bytes);
    if (threadIdx.x == 0)
        *flag_word = 1;
    __syncthreads();

    const int tid = threadIdx.x;
    const int tile_id = xcd_contiguous_tile((int)blockIdx.x, (int)gridDim.x);
    const int img_idx = tile_id / tiles_per_img;
    const int t_in_img = tile_id - img_idx * tiles_per_img;
    const int tile_y0 = (t_in_img / tiles_x) * TH;
    const int tile_x0 = (t_in_img % tiles_x) * kTileW;
    const size_t img = (size_t)img_idx * h * w;
    const int r4 = (radius + 3) & ~3;
    const int tlh = TH + 2 * radius;

    for (int i = tid; i < lut_len * LUTREP; i += NT)
        lutrep[i] = lut[i / LUTREP];
    for (int i = tid; i < (radius + 1) * sw_len; i += NT)
        swl[i] = swsym[i];
    int grey = 1;  // every src texel staged by this thread has B == G == R
    for (int item = tid; item < tlh * Q4; item += NT) {
        const int ry = item / Q4, k = item - ry * Q4;
        const int gy = border_interpolate(tile_y0 - radius + ry, h, border);
        uint32_t jv[4], sv[4];
        load_tile_quad(joint, src, img, gy, tile_x0 - r4 + 4 * k, w, jcn, SCN, border, jv, sv);
#pragma unroll
        for (int u = 0; u < 4; u++) {
            if (SCN == 3)
                grey &= (int)(((sv[u] ^ (sv[u] >> 8)) & 0xffffu) == 0u);
            tile[ry * TLW + u * Q4 + k] = make_uint2(jv[u], sv[u]);
        }
    }
    const int all_grey = block_all(grey, flag_word);  // also the barrier that publishes the tile
    if (flags & kJbfStageOnly)  // benchmark aid: staging only (tools/jbf_tune.py --stage-only)
        return;

    const int tx = tid & 15;
    const int ty = tid >> 4;
    const uint32_t lane_lut = (uint32_t)(tid & (LUTREP - 1));
    const uint32_t amax = (uint32_t)(lut_len - 1);
    uint32_t jc[kPix];
#pragma unroll
    for (int p = 0; p < kPix; p++) {
        const int X = 4 * tx + p + r4;
        jc[p] = tile[(ty + radius) * TLW + (X & 3) * Q4 + (X >> 2)].x;
    }
    const uint32_t lut_lane_addr = lds_addr(lutrep) + lane_lut * 4u;
    const uint32_t sw_addr0 = lds_addr(swl);
    const uint32_t tile_lane_addr = lds_addr(tile) + (uint32_t)tx * 8u;

    float sum[kPix][SCN];
    float wsum[kPix];
#pragma unroll
    for (int p = 0; p < kPix; p++) {
        wsum[p] = 0.f;
#pragma unroll
        for (int c = 0; c < SCN; c++)
            sum[p][c] = 0.f;
    }
    if (SCN == 3 && !all_grey) {
        jbf_tap_loop<SCN, LUTREP, CLAMP, TLW, 8>(lut_lane_addr, sw_addr0, tile_lane_addr, 0u, jc, amax,
                                              ty, radius, r4, sw_len, hwtab, sum, wsum);
    } else {
        // single-channel accumulation; for a grey 3-channel src the three sums are the same
        // sequence of float operations, so replicating one of them is bit-identical
        float sum1[kPix][1];
#pragma unroll
        for (int p = 0; p < kPix; p++)
            sum1[p][0] = 0.f;
        jbf_tap_loop<1, LUTREP, CLAMP, TLW, 8>(lut_lane_addr, sw_addr0, tile_lane_addr, 0u, jc, amax, ty,
                                            radius, r4, sw_len, hwtab, sum1, wsum);
#pragma unroll
        for (int p = 0; p < kPix; p++)
#pragma unroll
            for (int c = 0; c < SCN; c++)
                sum[p][c] = sum1[p][0];
    }

    store_quad<SCN, SCN>(dst, img, tile_y0 + ty, tile_x0 + 4 * tx, h, w, sum, wsum, flags);
}

// ------------------------------------------------------------------------------------------
// 64x64-tile kernel (1024 threads = 4 waves/SIMD), the default for radius <= 36.
//
// One launch shape serves both kinds of src; each tile decides for itself while staging:
//   * grey src (single-channel src, or every src texel of the tile has B = G = R -- the case of
//     the reference's `-r.png`): the tile is staged as 4-byte texels {B,G,R joint, grey src}.
//     That halves the tile (130 rows x 144 x 4 B = 73 KB), which is what lets a 64-row tile, a
//     32x replicated (conflict-free) LUT and - for the test aids - the weight table share 160 KB
//     of LDS, i.e. what buys 4 waves per SIMD.  All 1024 threads run the single-channel loop.
//   * colour src: a second plane of 2-byte texels {G src, R src} beside the grey-packed one (6 bytes
//     per texel), one pass on all 1024 threads where that fits with at least 8 LUT replicas (radius
//     33: 32 replicas; the reference's c15 s28 at pitch 176: 8); otherwise passes of 32 / 16 / 8
//     rows of the same two planes, run by threads 0 .. 16 * rows - 1 while all threads stage.
// The colour LUT sits at the END of the workgroup's 163,840-byte LDS allocation and holds only
// the entries before its zero tail: an index past the table addresses LDS beyond the
// allocation, where ds_read returns 0 -- exactly the LUT value there -- so the per-tap clamp
// disappears.  rf_jbf_u8 verifies that behaviour once per device with a probe kernel and uses
// the clamping kernel above if it ever does not hold.
// LDS: [flag][sw table: test aids only][tile ...     free ...][LUT nz*REP f32] = 163,840 B
// ------------------------------------------------------------------------------------------
constexpr int kT64Lds = 163840;

// One tile of a ragged launch (rf_jbf_ragged_u8: images of different sizes packed one after
// another): where its image starts in the packed buffers, the image's size and the tile's origin.
// Written by the host, one per workgroup, indexed by the xcd_contiguous_tile id.
struct alignas(16) JbfTileRec {
    unsigned long long first;  // pixels before the image
    int h, w, tile_y0, tile_x0, pad[2];
};
static_assert(sizeof(JbfTileRec) == 32, "the workspace holds 32 bytes per tile");

// The tiles argument of jbf_tile64_kernel and jbf_slab_kernel: tiles per image row (uniform launch: every image is
// h x w), or the tile records (ragged launch; h, w, tiles_per_img, y_base, x_base are unused).
template <bool kRagged>
struct JbfTilesArg {
    using type = int;
};
template <>
struct JbfTilesArg<true> {
    using type = const JbfTileRec *__restrict__;
};

// The last argument of jbf_tile64_kernel: nothing, or (kFlagged: the colour-tile launch of the
// two-workgroups-per-CU route, jbf_tile64x2_kernel below) one vote byte per tile - the workgroup of a
// tile whose bit 0 is clear (a grey src) leaves at once.
struct JbfNoTileFlags {};
template <bool kFlagged>
struct JbfTileFlagsArg {
    using type = JbfNoTileFlags;
};
template <>
struct JbfTileFlagsArg<true> {
    using type = const uint8_t *__restrict__;
};

// TH = tile rows: 64 (64x64 tile), or 32 / 16 for the 32x128 and 16x256 strips that cover the
// last h % 64 rows (same 1024 lanes, same tap loops, less padding; 3-channel sources only have
// the 32-row strip, whose colour tile still fits the LDS in one pass).
template <int SCN, int GREP, int CREP, int TLW, int TH = 64, bool kRagged = false, bool kFlagged = false>
__global__ __launch_bounds__(1024) void jbf_tile64_kernel(
    const uint8_t *__restrict__ joint, const uint8_t *__restrict__ src, uint8_t *__restrict__ dst,
    int h, int w, int jcn, int radius, int border, const float *__restrict__ lut, int nz,
    const int *__restrict__ hwtab, const float *__restrict__ swsym, int sw_len,
    typename JbfTilesArg<kRagged>::type tiles_x, int tiles_per_img, int flags, int crows, int y_base,
    int x_base, typename JbfTileFlagsArg<kFlagged>::type tile_flags)
{
    if constexpr (kFlagged) {
        // (the same tile index as the first launch gave this workgroup: same grid, same mapping)
        if ((tile_flags[xcd_contiguous_tile((int)blockIdx.x, (int)gridDim.x)] & 1) == 0)
            return;
    }
    constexpr int NT = 1024;
    constexpr int QW = NT / TH;   // lanes (4-pixel quads) per tile row
    constexpr int TW = 4 * QW;    // tile width
    static_assert(TH == 64 || TH == 32 || ((TH == 16 || TH == 128) && SCN == 1), "tile shapes");
    // a half-wave covers 32/QW tile rows of QW consecutive words each: the pitch must spread
    // those rows over disjoint banks
    static_assert(QW >= 32 || (QW == 16 && TLW % 32 == 16) || (QW == 8 && TLW % 32 == 8),
                  "row pitch keeps the rows of a half-wave on disjoint banks");
    constexpr int Q4 = TLW / 4;
    extern __shared__ __align__(16) unsigned char smem[];
    volatile int *flag_word = reinterpret_cast<volatile int *>(smem);
    // (the asm tap loops take their weights through scalar loads: the LDS copy of the weight table is
    //  staged only for the compiler-scheduled loop and the round-4 loop, the test / A-B aids)
    const bool need_sw = (flags & (kJbfCompilerLoop | kJbfLookahead1)) != 0;
    float *swl = reinterpret_cast<float *>(smem + 16);
    const int sw_bytes = need_sw ? ((radius + 1) * sw_len * 4 + 15) & ~15 : 0;
    unsigned char *tile_raw = smem + 16 + sw_bytes;
    if (threadIdx.x == 0)
        *flag_word = 3;
    __syncthreads();

    const int tid = threadIdx.x;
    const int tile_id = xcd_contiguous_tile((int)blockIdx.x, (int)gridDim.x);
    int tile_y0, tile_x0;
    size_t img;
    if constexpr (kRagged) {
        // one record per workgroup: the same words in every lane (scalar loads, scalar registers)
        const JbfTileRec *rec = tiles_x + tile_id;
        img = (size_t)rec->first;
        h = rec->h;
        w = rec->w;
        tile_y0 = rec->tile_y0;
        tile_x0 = rec->tile_x0;
    } else {
        const int img_idx = tile_id / tiles_per_img;
        const int t_in_img = tile_id - img_idx * tiles_per_img;
        tile_y0 = y_base + (t_in_img / tiles_x) * TH;
        tile_x0 = x_base + (t_in_img % tiles_x) * TW;
        img = (size_t)img_idx * h * w;
    }
    const int r4 = (radius + 3) & ~3;
    const int tx = tid % QW;
    const int ty = tid / QW;

    // ---- weight table, grey LUT (optimistic), grey-packed tile ----
    if (need_sw)
        for (int i = tid; i < (radius + 1) * sw_len; i += NT)
            swl[i] = swsym[i];
    float *lut_g = reinterpret_cast<float *>(smem + kT64Lds - nz * GREP * 4);
    for (int i = tid; i < nz * GREP; i += NT)
        lut_g[i] = lut[i / GREP];
    uint32_t *tile4 = reinterpret_cast<uint32_t *>(tile_raw);
    int grey = 1, grey_joint = 1;
    // Single-channel (or grey 3-channel) joint together with a single-channel (or grey) src: the
    // joint field of a texel holds the value times the LUT's byte stride (3x unless the joint
    // really is one channel: the colour distance of three equal channels is 3|d|), which turns
    // the SAD of the tap loop into the gather address (jbf_tap_loop_grey4<.., J1 = true>).
    // Known up front for 1-channel buffers (j1): staged in that form.  For 3-channel buffers
    // it is found out per tile, and the staged tile is then rewritten in LDS.
    const bool j1_ok = !(flags & kJbfCompilerLoop);
    const bool j1 = SCN == 1 && jcn != 3 && j1_ok;
    const uint32_t j1_scale = (uint32_t)(jcn == 1 ? 1 : 3) * (GREP * 4u);
    const int tlh = TH + 2 * radius;
    // one work item = 4 consecutive tile columns (4k..4k+3) of one tile row
    for (int item = tid; item < tlh * Q4; item += NT) {
        const int ry = item / Q4, k = item - ry * Q4;
        const int gy = border_interpolate(tile_y0 - radius + ry, h, border);
        uint32_t jv[4], sv[4];
        load_tile_quad(joint, src, img, gy, tile_x0 - r4 + 4 * k, w, jcn, SCN, border, jv, sv);
#pragma unroll
        for (int u = 0; u < 4; u++) {
            if (SCN == 3)
                grey &= (int)(((sv[u] ^ (sv[u] >> 8)) & 0xffffu) == 0u);
            if (jcn == 3)
                grey_joint &= (int)(((jv[u] ^ (jv[u] >> 8)) & 0xffffu) == 0u);
            const uint32_t jfield = j1 ? (jv[u] & 0xffu) * j1_scale : jv[u];
            tile4[ry * TLW + u * Q4 + k] = jfield | (sv[u] << 24);
        }
    }
    // (the barrier inside also publishes sw table, LUT and tile)
    const int grey_bits = block_all2(grey, grey_joint, const_cast<int *>(flag_word));
    const int all_grey = grey_bits & 1;
    if (flags & kJbfStageOnly)  // benchmark aid: staging only (tools/jbf_tune.py --stage-only)
        return;
    // grey src and grey joint found out only now: rewrite the joint fields in place
    const bool j1_late = !j1 && j1_ok && (SCN == 1 || all_grey) && (grey_bits & 2);
    if (j1_late) {
        for (int idx = tid; idx < tlh * TLW; idx += NT) {
            const uint32_t t = tile4[idx];
            tile4[idx] = (t & 0xffu) * j1_scale | (t & 0xff000000u);
        }
        __syncthreads();
    }

    const uint32_t sw_addr0 = lds_addr(swl);
    if (SCN == 1 || all_grey) {
        uint32_t jc[kPix];
#pragma unroll
        for (int p = 0; p < kPix; p++) {
            const int X = 4 * tx + p + r4;
            jc[p] = tile4[(ty + radius) * TLW + (X & 3) * Q4 + (X >> 2)] & 0x00ffffffu;
        }
        float sum1[kPix][1], wsum[kPix];
#pragma unroll
        for (int p = 0; p < kPix; p++) {
            sum1[p][0] = 0.f;
            wsum[p] = 0.f;
        }
        const uint32_t lut_lane_addr = lds_addr(lut_g) + (uint32_t)(tid & (GREP - 1)) * 4u;
        const uint32_t tile_lane_addr = lds_addr(tile4) + (uint32_t)tx * 4u;
        if (flags & kJbfCompilerLoop)  // benchmark aid: compiler-scheduled loop instead of the asm one
            jbf_tap_loop<1, GREP, false, TLW, 4>(lut_lane_addr, sw_addr0, tile_lane_addr, 0u, jc, 0u,
                                                 ty, radius, r4, sw_len, hwtab, sum1, wsum);
        else if (flags & kJbfLookahead1) {  // A/B aid: the round-4 pipeline depth
            if (j1 || j1_late)
                jbf_tap_loop_grey4<GREP, TLW, true>(lut_lane_addr, sw_addr0, tile_lane_addr, jc, ty,
                                                    radius, r4, sw_len, hwtab, sum1, wsum);
            else
                jbf_tap_loop_grey4<GREP, TLW>(lut_lane_addr, sw_addr0, tile_lane_addr, jc, ty, radius,
                                              r4, sw_len, hwtab, sum1, wsum);
        } else if (j1 || j1_late)
            jbf_tap_loop_grey4_la2<GREP, TLW, true>(lut_lane_addr, swsym, tile_lane_addr, jc, ty,
                                                    radius, r4, sw_len, hwtab, sum1, wsum);
        else if (!(flags & kJbfNoMsad) && jbf_wave_takes_msad(jc))  // (per wave: no centre with a zero channel)
            jbf_tap_loop_grey4_la2<GREP, TLW, false, false, true>(lut_lane_addr, swsym, tile_lane_addr, jc,
                                                                  ty, radius, r4, sw_len, hwtab, sum1, wsum);
        else
            jbf_tap_loop_grey4_la2<GREP, TLW>(lut_lane_addr, swsym, tile_lane_addr, jc, ty, radius,
                                              r4, sw_len, hwtab, sum1, wsum);
        store_quad<1, SCN>(dst, img, tile_y0 + ty, tile_x0 + 4 * tx, h, w, sum1, wsum, flags);
        return;
    }

    if constexpr (SCN == 3) {
        if (crows == TH) {
            // ---- colour src, one pass: the grey-packed plane already holds {B,G,R joint, B src};
            //      a second plane of 2-byte texels adds {G src, R src}: 6 bytes per texel, all
            //      1024 threads stay busy (4 waves/SIMD) ----
            uint16_t *plane_b = reinterpret_cast<uint16_t *>(tile_raw + (size_t)tlh * TLW * 4);
            float *lut_c = reinterpret_cast<float *>(smem + kT64Lds - nz * CREP * 4);
            __syncthreads();  // the grey LUT region is about to be overwritten
            for (int i = tid; i < nz * CREP; i += NT)
                lut_c[i] = lut[i / CREP];
            for (int item = tid; item < tlh * Q4; item += NT) {
                const int ry = item / Q4, k = item - ry * Q4;
                const int gy = border_interpolate(tile_y0 - radius + ry, h, border);
                uint32_t jv[4], sv[4];
                load_tile_quad(joint, src, img, gy, tile_x0 - r4 + 4 * k, w, jcn, 3, border, jv, sv);
#pragma unroll
                for (int u = 0; u < 4; u++)
                    plane_b[ry * TLW + u * Q4 + k] = (uint16_t)(sv[u] >> 8);
            }
            __syncthreads();
            uint32_t jc[kPix];
#pragma unroll
            for (int p = 0; p < kPix; p++) {
                const int X = 4 * tx + p + r4;
                jc[p] = tile4[(ty + radius) * TLW + (X & 3) * Q4 + (X >> 2)] & 0x00ffffffu;
            }
            float sum[kPix][3], wsum[kPix];
#pragma unroll
            for (int p = 0; p < kPix; p++) {
                wsum[p] = 0.f;
                sum[p][0] = sum[p][1] = sum[p][2] = 0.f;
            }
            const uint32_t lut_lane_addr = lds_addr(lut_c) + (uint32_t)(tid & (CREP - 1)) * 4u;
            if (flags & kJbfCompilerLoop)  // test aid: compiler-scheduled loop instead of the asm one
                jbf_tap_loop<3, CREP, false, TLW, 6>(lut_lane_addr, sw_addr0,
                                                     lds_addr(tile4) + (uint32_t)tx * 4u,
                                                     lds_addr(plane_b) + (uint32_t)tx * 2u, jc, 0u,
                                                     ty, radius, r4, sw_len, hwtab, sum, wsum);
            else if (!(flags & kJbfNoMsad) && jbf_wave_takes_msad(jc))
                jbf_tap_loop_rgb6<CREP, TLW, false, true>(lut_lane_addr, swsym,
                                                          lds_addr(tile4) + (uint32_t)tx * 4u,
                                                          lds_addr(plane_b) + (uint32_t)tx * 2u, jc, ty,
                                                          radius, r4, sw_len, hwtab, sum, wsum);
            else
                jbf_tap_loop_rgb6<CREP, TLW>(lut_lane_addr, swsym,
                                             lds_addr(tile4) + (uint32_t)tx * 4u,
                                             lds_addr(plane_b) + (uint32_t)tx * 2u, jc, ty, radius,
                                             r4, sw_len, hwtab, sum, wsum);
            store_quad<3, 3>(dst, img, tile_y0 + ty, tile_x0 + 4 * tx, h, w, sum, wsum, flags);
            return;
        }
        if constexpr (TH != 64)
            return;  // strips are only launched when the one-pass colour tile fits
        // ---- colour src whose one-pass tile does not fit (row pitch 176: radius 37..52, e.g. the
        //      reference's c15 s28 -> radius 42 on a colour reflectance, /root/reference/README.md:64):
        //      64/crows passes of crows rows, the same two planes of 6 bytes per texel and the same
        //      asm tap loop as the one-pass form, run by threads 0 .. 16*crows-1 while all threads
        //      stage.  (Round 3 had 8-byte texels here, which only left room for 16-row passes at
        //      radius 42 and ran the compiler-scheduled loop: 3.9x the time per tap of the radius-33
        //      colour loop, profiles/r04_bench_other.json.) ----
        float *lut_c = reinterpret_cast<float *>(smem + kT64Lds - nz * CREP * 4);
        const int tlh8 = crows + 2 * radius;
        uint16_t *plane_b = reinterpret_cast<uint16_t *>(tile_raw + (size_t)tlh8 * TLW * 4);
        for (int half = 0; half * crows < 64; half++) {
            const int y0 = tile_y0 + crows * half;
            if (y0 >= h)
                break;
            __syncthreads();  // everyone is done with the previous contents of the tile
            if (half == 0)
                for (int i = tid; i < nz * CREP; i += NT)
                    lut_c[i] = lut[i / CREP];
            for (int item = tid; item < tlh8 * Q4; item += NT) {
                const int ry = item / Q4, k = item - ry * Q4;
                const int gy = border_interpolate(y0 - radius + ry, h, border);
                uint32_t jv[4], sv[4];
                load_tile_quad(joint, src, img, gy, tile_x0 - r4 + 4 * k, w, jcn, 3, border, jv, sv);
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    tile4[ry * TLW + u * Q4 + k] = jv[u] | (sv[u] << 24);
                    plane_b[ry * TLW + u * Q4 + k] = (uint16_t)(sv[u] >> 8);
                }
            }
            __syncthreads();
            if (tid < 16 * crows) {
                uint32_t jc[kPix];
#pragma unroll
                for (int p = 0; p < kPix; p++) {
                    const int X = 4 * tx + p + r4;
                    jc[p] = tile4[(ty + radius) * TLW + (X & 3) * Q4 + (X >> 2)] & 0x00ffffffu;
                }
                float sum[kPix][3], wsum[kPix];
#pragma unroll
                for (int p = 0; p < kPix; p++) {
                    wsum[p] = 0.f;
                    sum[p][0] = sum[p][1] = sum[p][2] = 0.f;
                }
                const uint32_t lut_lane_addr = lds_addr(lut_c) + (uint32_t)(tid & (CREP - 1)) * 4u;
                if (flags & kJbfCompilerLoop)  // test aid: compiler-scheduled loop instead of the asm one
                    jbf_tap_loop<3, CREP, false, TLW, 6>(lut_lane_addr, sw_addr0,
                                                         lds_addr(tile4) + (uint32_t)tx * 4u,
                                                         lds_addr(plane_b) + (uint32_t)tx * 2u, jc, 0u,
                                                         ty, radius, r4, sw_len, hwtab, sum, wsum);
                else if (!(flags & kJbfNoMsad) && jbf_wave_takes_msad(jc))
                    jbf_tap_loop_rgb6<CREP, TLW, false, true>(lut_lane_addr, swsym,
                                                              lds_addr(tile4) + (uint32_t)tx * 4u,
                                                              lds_addr(plane_b) + (uint32_t)tx * 2u, jc,
                                                              ty, radius, r4, sw_len, hwtab, sum, wsum);
                else
                    jbf_tap_loop_rgb6<CREP, TLW>(lut_lane_addr, swsym,
                                                 lds_addr(tile4) + (uint32_t)tx * 4u,
                                                 lds_addr(plane_b) + (uint32_t)tx * 2u, jc, ty, radius,
                                                 r4, sw_len, hwtab, sum, wsum);
                store_quad<3, 3>(dst, img, y0 + ty, tile_x0 + 4 * tx, h, w, sum, wsum, flags);
            }
        }
    }
}

// One channel of a 3-channel result: the lane's 4 horizontally adjacent outputs of channel c.
__device__ inline void store_quad_channel(uint8_t *dst, size_t img, int oy, int ox0, int h, int w,
                                          int c, const float (&sum)[kPix][1],
                                          const float (&wsum)[kPix], int flags)
{
    if (oy >= h || ox0 >= w)
        return;
    uint8_t *o = dst + (img + (size_t)oy * w + ox0) * 3 + c;
#pragma unroll
    for (int p = 0; p < kPix; p++) {
        if (ox0 + p >= w)
            break;
        const float d = (flags & RF_JBF_TRUE_DIVISION) ? wsum[p] : __fdiv_rn(1.0f, wsum[p]);
        o[p * 3] = saturate_u8(finish_value(sum[p][0], d, flags));
    }
}

// Probe for the "LDS reads beyond the allocation return 0" behaviour the 64x64 kernel relies on.
__global__ void lds_oob_probe_kernel(uint32_t *out)
{
    extern __shared__ __align__(16) unsigned char smem[];
    uint32_t *w = reinterpret_cast<uint32_t *>(smem);
    for (int i = threadIdx.x; i < kT64Lds / 4; i += blockDim.x)
        w[i] = 0xdeadbeefu;
    __syncthreads();
    uint32_t bad = 0;
    const uint32_t addrs[4] = {(uint32_t)kT64Lds + 4u * threadIdx.x, (uint32_t)kT64Lds + 61056u,
                               262140u, (uint32_t)kT64Lds - 4u};
#pragma unroll
    for (int k = 0; k < 4; k++) {
        uint32_t v;
        asm volatile("ds_read_b32 %0, %1\n s_waitcnt lgkmcnt(0)" : "=v"(v) : "v"(addrs[k]));
        bad |= (k < 3) ? (v != 0u) : (v != 0xdeadbeefu);
    }
    if (bad)
        atomicOr(out, 1u);
}

// LDS of a workgroup of jbf_tile64x2_kernel (below): half of a CU's, so that two are resident.
constexpr int kT64x2Lds = 81920;

// The same probe for an allocation of half the LDS with a second workgroup resident on the CU: a read
// beyond the workgroup's own allocation must return 0 although the address lies inside the CU's LDS,
// where the neighbour (or, the LDS not being cleared between workgroups, an earlier one) has written
// the pattern.  Launched with several workgroups per CU slot.
__global__ __launch_bounds__(256) void lds_oob_probe_half_kernel(uint32_t *out)
{
    extern __shared__ __align__(16) unsigned char smem[];
    uint32_t *w = reinterpret_cast<uint32_t *>(smem);
    for (int i = threadIdx.x; i < kT64x2Lds / 4; i += blockDim.x)
        w[i] = 0xdeadbeefu;
    __syncthreads();
    uint32_t bad = 0;
    const uint32_t addrs[5] = {(uint32_t)kT64x2Lds + 4u * threadIdx.x, (uint32_t)kT64x2Lds + 61056u,
                               (uint32_t)kT64Lds - 4u, 262140u, (uint32_t)kT64x2Lds - 4u};
#pragma unroll
    for (int k = 0; k < 5; k++) {
        uint32_t v;
        asm volatile("ds_read_b32 %0, %1\n s_waitcnt lgkmcnt(0)" : "=v"(v) : "v"(addrs[k]));
        bad |= (k < 4) ? (v != 0u) : (v != 0xdeadbeefu);
    }
    if (bad)
        atomicOr(out, 2u);
}

struct Tiled2Config {
    int th, lutrep;
    bool full_lut;  // stage all 256*jcn LUT entries and skip the per-tap clamp
};

size_t tiled2_lds_bytes(const JbfTables &t, int th, int lutrep, bool full_lut)
{
    const int lut_len = full_lut ? 256 * t.joint_cn : t.lut_len;
    const size_t lut_bytes = ((size_t)lut_len * lutrep * 4 + 15) & ~(size_t)15;
    const size_t sw_bytes = ((size_t)(t.radius + 1) * t.sw_len * 4 + 15) & ~(size_t)15;
    return 16 + lut_bytes + sw_bytes + (size_t)kTlw2 * (th + 2 * t.radius) * sizeof(uint2);
}

template <int SCN, int TH, int LUTREP>
int launch_tiled2(const JbfTables &t, bool full_lut, const uint8_t *joint, const uint8_t *src,
                  uint8_t *dst, int n, int h, int w, int jcn, int border, int flags,
                  hipStream_t stream)
{
    const int lut_len = full_lut ? 256 * t.joint_cn : t.lut_len;
    const bool clamp = lut_len < 256 * t.joint_cn;
    const size_t lds = tiled2_lds_bytes(t, TH, LUTREP, full_lut);
    const int tiles_x = ceil_div(w, kTileW), tiles_y = ceil_div(h, TH);
    const long long blocks = (long long)tiles_x * tiles_y * n;
    if (!launch_fits(blocks, 16 * TH))
        return fail(RF_E_UNSUPPORTED, "rf_jbf_u8: batch too large for one launch");
    auto kern = clamp ? jbf_tiled2_kernel<SCN, TH, LUTREP, true>
                      : jbf_tiled2_kernel<SCN, TH, LUTREP, false>;
    RF_HIP_CHECK(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)lds));
    hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(16 * TH), lds, stream, joint, src, dst, h,
                       w, jcn, t.radius, border, t.d_lut, lut_len, t.d_hw, t.d_swsym, t.sw_len,
                       tiles_x, tiles_x * tiles_y, flags);
    return RF_OK;
}


std::mutex g_oob_mu;
std::vector<int> g_oob_ok;  // per device: -1 unknown, 0 no, 1 yes (guarded by g_oob_mu)

// Runs the probes once per device.  Synchronises the device (only on the first JBF call).
// *ok: the rule holds for a workgroup that owns the whole LDS; *ok_half (if asked for): also for one
// of two workgroups that own half of it each.
int lds_oob_reads_zero(int dev, bool *ok, bool *ok_half = nullptr)
{
    {
        std::lock_guard<std::mutex> lock(g_oob_mu);
        if ((int)g_oob_ok.size() <= dev)
            g_oob_ok.resize(dev + 1, -1);
        if (g_oob_ok[dev] >= 0) {
            *ok = (g_oob_ok[dev] & 1) != 0;
            if (ok_half)
                *ok_half = (g_oob_ok[dev] & 2) != 0;
            return RF_OK;
        }
    }
    // once per device and process, on a stream of its own, waited for here: the answer selects
    // kernels.  (The caller's stream may be capturing: CaptureRelax admits the allocation and the
    // wait on this OTHER stream; nothing of the probe enters the caller's graph.)
    CaptureRelax relax;
    uint32_t *d_flag = nullptr;
    hipStream_t ps = nullptr;
    RF_HIP_CHECK(hipStreamCreateWithFlags(&ps, hipStreamNonBlocking));
    struct StreamGuard {
        hipStream_t s;
        ~StreamGuard() { (void)hipStreamDestroy(s); }
    } guard{ps};
    RF_HIP_CHECK(hipMalloc(&d_flag, sizeof(uint32_t)));
    RF_HIP_CHECK(hipMemsetAsync(d_flag, 0, sizeof(uint32_t), ps));
    RF_HIP_CHECK(hipFuncSetAttribute((const void *)lds_oob_probe_kernel,
                                     hipFuncAttributeMaxDynamicSharedMemorySize, kT64Lds));
    hipLaunchKernelGGL(lds_oob_probe_kernel, dim3(8), dim3(256), kT64Lds, ps, d_flag);
    RF_HIP_CHECK(hipFuncSetAttribute((const void *)lds_oob_probe_half_kernel,
                                     hipFuncAttributeMaxDynamicSharedMemorySize, kT64x2Lds));
    hipLaunchKernelGGL(lds_oob_probe_half_kernel, dim3(2048), dim3(256), kT64x2Lds, ps, d_flag);
    uint32_t flag = 3;
    RF_HIP_CHECK(hipMemcpyAsync(&flag, d_flag, sizeof(flag), hipMemcpyDeviceToHost, ps));
    RF_HIP_CHECK(hipStreamSynchronize(ps));
    (void)hipFree(d_flag);
    std::lock_guard<std::mutex> lock(g_oob_mu);
    g_oob_ok[dev] = (int)(~flag & 3u);  // bit 0: whole-LDS probe passed, bit 1: half-LDS probe passed
    *ok = (flag & 1u) == 0;
    if (ok_half)
        *ok_half = (flag & 2u) == 0;
    return RF_OK;
}

// LDS needed by jbf_tile64_kernel for grey / colour tiles with the given LUT replication.
// Rows per colour pass that fit (64 = one pass with 6-byte texels; 32, 16, 8 = passes with
// 8-byte texels), or 0.
int tile64_fits(const JbfTables &t, int nz, int grep, int crep, int scn, int tlw, int th, int flags)
{
    if (2 * t.r4 + 4 * (1024 / th) + 8 > tlw)
        return 0;
    const bool need_sw = (flags & (kJbfCompilerLoop | kJbfLookahead1)) != 0;  // as in the kernel
    const size_t sw_bytes =
        16 + (need_sw ? ((size_t)(t.radius + 1) * t.sw_len * 4 + 15) & ~(size_t)15 : 0);
    const size_t grey = sw_bytes + (size_t)tlw * (th + 2 * t.radius) * 4 + (size_t)nz * grep * 4;
    if (grey > (size_t)kT64Lds)
        return 0;
    if (scn == 1)
        return 32;
    // colour tiles in one pass: a 4-byte and a 2-byte plane of the full tile
    if (sw_bytes + (size_t)tlw * (th + 2 * t.radius) * 6 + (size_t)nz * crep * 4 <= (size_t)kT64Lds)
        return th;
    if (th != 64)
        return 0;
    for (int crows = 32; crows >= 8; crows >>= 1) {
        const size_t col =
            sw_bytes + (size_t)tlw * (crows + 2 * t.radius) * 6 + (size_t)nz * crep * 4;
        if (col <= (size_t)kT64Lds)
            return crows;
    }
    return 0;
}

// Rows [y_base, y_base + rows) of every image, in tiles of TH rows.
template <int SCN, int GREP, int CREP, int TLW, int TH = 64>
int launch_tile64(const JbfTables &t, int nz, int crows, const uint8_t *joint, const uint8_t *src,
                  uint8_t *dst, int n, int h, int w, int jcn, int border, int flags,
                  hipStream_t stream, int y_base = 0, int rows = -1, int x_base = 0, int cols = -1)
{
    if (rows < 0)
        rows = h;
    if (cols < 0)
        cols = w;
    const int tiles_x = ceil_div(cols, 4 * (1024 / TH)), tiles_y = ceil_div(rows, TH);
    const long long blocks = (long long)tiles_x * tiles_y * n;
    if (!launch_fits(blocks, 1024))
        return fail(RF_E_UNSUPPORTED, "rf_jbf_u8: batch too large for one launch");
    auto kern = jbf_tile64_kernel<SCN, GREP, CREP, TLW, TH>;
    RF_HIP_CHECK(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize,
                                     kT64Lds));
    hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(1024), kT64Lds, stream, joint, src, dst,
                       h, w, jcn, t.radius, border, t.d_lut, nz, t.d_hw, t.d_swsym, t.sw_len,
                       tiles_x, tiles_x * tiles_y, flags, crows, y_base, x_base, JbfNoTileFlags{});
    return RF_OK;
}

// Radius <= 36: 64x64 tiles, except that the last h % 64 rows go to one 32x128 and/or one 16x256
// strip of tiles, and the last w % 64 columns to a column of 128x32 tiles, whenever that takes
// fewer workgroups than another row / column of 64x64 tiles (every workgroup costs the same
// 1024 lanes x all taps).  3-channel sources only have the 32x128 strip, whose colour tile still
// fits the LDS in one pass.  Strips may overlap at the bottom right corner: both write the same
// bytes.
// The areas of an h x w image: 64x64 tiles cover [0, rows_main) x [0, cols_main), the 32x128 strip
// the s32 rows below them, the 16x256 strip the s16 rows below that, the 128x32 strip the last sx
// columns over all h rows.  Decided here for the uniform launches and the ragged ones alike.
struct Tile64Areas {
    int rows_main, cols_main, s32, s16, sx;
};

Tile64Areas tile64_areas(const JbfTables &t, int nz, int grep, int crep, int scn, int flags, int h,
                         int w)
{
    const bool only64 = (flags & kJbfTile64Only) != 0;  // benchmark / test aid: 64x64 tiles only
    // ---- right strip (single-channel sources)
    int sx = 0;
    if (scn == 1 && !only64 && (w & 63) > 0 && (w & 63) <= 32 &&
        tile64_fits(t, nz, grep, crep, scn, 136, 128, flags) > 0 && ceil_div(h, 128) < ceil_div(h, 64))
        sx = w & 63;
    const int cols_main = w - sx;
    // ---- bottom strips
    const int rem = h & 63;
    const bool ok32 = tile64_fits(t, nz, grep, crep, scn, 208, 32, flags) > 0;
    const bool ok16 = scn == 1 && tile64_fits(t, nz, grep, crep, scn, 336, 16, flags) > 0;
    int s32 = 0, s16 = 0;  // rows given to each strip
    if (rem > 0 && rem <= 16 && ok16)
        s16 = rem;
    else if (rem > 0 && rem <= 32 && ok32)
        s32 = rem;
    else if (rem > 32 && rem <= 48 && ok32 && ok16)
        s32 = 32, s16 = rem - 32;
    const int strip_blocks =
        (s32 ? ceil_div(cols_main, 128) : 0) + (s16 ? ceil_div(cols_main, 256) : 0);
    if (only64 || cols_main == 0 || ((s32 || s16) && strip_blocks >= ceil_div(cols_main, 64)))
        s32 = s16 = 0;
    return Tile64Areas{h - s32 - s16, cols_main, s32, s16, sx};
}

template <int SCN, int GREP, int CREP>
int launch_tile64_rows(const JbfTables &t, int nz, int crows, const uint8_t *joint,
                       const uint8_t *src, uint8_t *dst, int n, int h, int w, int jcn, int border,
                       int flags, hipStream_t stream, bool strips_only = false)
{
    // (strips_only: the 64x64 tiles of the main area have been launched by the two-per-CU route)
    const Tile64Areas a = tile64_areas(t, nz, GREP, CREP, SCN, flags, h, w);
    const int rows_main = a.rows_main, cols_main = a.cols_main, s32 = a.s32, s16 = a.s16, sx = a.sx;
    int rc = RF_OK;
    if (rows_main > 0 && cols_main > 0 && !strips_only)
        rc = launch_tile64<SCN, GREP, CREP, 144>(t, nz, crows, joint, src, dst, n, h, w, jcn,
                                                 border, flags, stream, 0, rows_main, 0, cols_main);
    if (rc == RF_OK && s32)
        rc = launch_tile64<SCN, GREP, CREP, 208, 32>(t, nz, 32, joint, src, dst, n, h, w, jcn,
                                                     border, flags, stream, rows_main, s32, 0,
                                                     cols_main);
    if constexpr (SCN == 1) {
        if (rc == RF_OK && s16)
            rc = launch_tile64<1, GREP, CREP, 336, 16>(t, nz, 32, joint, src, dst, n, h, w, jcn,
                                                       border, flags, stream, rows_main + s32, s16,
                                                       0, cols_main);
        if (rc == RF_OK && sx)
            rc = launch_tile64<1, GREP, CREP, 136, 128>(t, nz, 32, joint, src, dst, n, h, w, jcn,
                                                        border, flags, stream, 0, h, cols_main, sx);
    }
    return rc;
}

// The tile shapes jbf_tile64_kernel is instantiated for, in order of preference:
// X(grey LUT replicas, colour LUT replicas, row pitch).  Row pitch 144 serves radius <= 36, 176
// radius <= 52 (colour tiles of the wide pitch run in 16- or 8-row passes).
#define RF_T64_SHAPES(X)                                                                          \
    X(32, 32, 144) X(32, 16, 144) X(16, 8, 144) X(8, 4, 144) X(32, 16, 176) X(32, 8, 176)         \
    X(32, 4, 176) X(16, 8, 176) X(8, 4, 176)

struct Tile64Shape {
    int grep, crep, tlw, crows;  // crows: rows per colour pass (tile64_fits)
};

// The shape a call runs at; it depends on the tables, not on the image sizes.  False: none fits.
// A colour src first looks for a shape whose colour tile fits in ONE pass over the 64 rows,
// on all 1024 lanes, even with fewer LUT replicas - down to 8 - (the reference's c15 s28,
// README.md:64, at pitch 176: 8 replicas, +3.5 % over two 32-row passes on half the lanes
// with 16), then for one that needs passes.
bool tile64_choose(const JbfTables &t, int nz, int src_cn, int flags, Tile64Shape *out)
{
    for (int min_rows = src_cn == 3 ? 64 : 1; min_rows >= 1; min_rows = min_rows == 64 ? 1 : 0) {
#define RF_T64_TRY(G_, C_, W_)                                                                    \
    if ((min_rows < 64 || C_ >= 8) && tile64_fits(t, nz, G_, C_, src_cn, W_, 64, flags) >= min_rows) { \
        *out = Tile64Shape{G_, C_, W_, tile64_fits(t, nz, G_, C_, src_cn, W_, 64, flags)};        \
        return true;                                                                              \
    }
        RF_T64_SHAPES(RF_T64_TRY)
#undef RF_T64_TRY
    }
    return false;
}

// What a launch of jbf_slab_kernel (radius 53..468, below) runs at: row pitch, LUT replicas, rows
// per band and per slab with 4-byte texels (crows_g, slab_g) and with 6-byte texels (crows_c,
// slab_c; crows_c = 0: one grey pass per channel).
struct SlabShape {
    int tlw, grep, crows_g, slab_g, crows_c, slab_c;
};
bool slab_choose(const JbfTables &t, int nz, int src_cn, SlabShape *out);

// ---- ragged form (rf_jbf_ragged_u8) ------------------------------------------------------------
// The tile classes of a ragged call in launch order: {tile rows, row pitch}; tile columns = 4096 / rows.
constexpr int kRaggedClasses = 4;
constexpr int kRaggedTh[kRaggedClasses] = {64, 32, 16, 128};
constexpr int kRaggedPitch144[kRaggedClasses] = {144, 208, 336, 136};

// What a ragged call launches: the shape (once per call) and, per tile class, the records of all
// images' tiles in image order.  tile64_areas decides per image, as for a uniform launch.
// Radius 53..468 (slab): one launch of jbf_slab_kernel over recs[0], every image's 64x64 tiles.
struct RaggedPlan {
    bool tiled = false;  // neither tiled nor slab: the entry falls back to one uniform call per image
    bool slab = false;
    Tile64Shape shape{};
    SlabShape slab_shape{};
    std::vector<JbfTileRec> recs[kRaggedClasses];
};

void plan_ragged(const JbfTables &t, int n, const int *heights, const int *widths, int src_cn,
                 int flags, int tune, RaggedPlan *plan)
{
    const int nz = t.lut_len < 256 * t.joint_cn ? t.lut_len - 1 : t.lut_len;
    if ((flags & RF_JBF_FORCE_GENERIC) || tune != 0)
        return;
    plan->tiled = tile64_choose(t, nz, src_cn, flags, &plan->shape);
    // no 64-row-tile shape holds the radius: tap-row slabs, as the uniform entry chooses them
    plan->slab = !plan->tiled && slab_choose(t, nz, src_cn, &plan->slab_shape);
    if (!plan->tiled && !plan->slab)
        return;
    const Tile64Shape &s = plan->shape;
    unsigned long long first = 0;
    for (int i = 0; i < n; i++) {
        const int h = heights[i], w = widths[i];
        Tile64Areas a{h, w, 0, 0, 0};  // the wide pitch and the slabs have 64x64 tiles alone
        if (plan->tiled && s.tlw == 144)
            a = tile64_areas(t, nz, s.grep, s.crep, src_cn, flags, h, w);
        // {y_base, rows, x_base, cols} of each class's area, as launch_tile64_rows hands them on
        const int area[kRaggedClasses][4] = {{0, a.rows_main, 0, a.cols_main},
                                             {a.rows_main, a.s32, 0, a.cols_main},
                                             {a.rows_main + a.s32, a.s16, 0, a.cols_main},
                                             {0, a.sx ? h : 0, a.cols_main, a.sx}};
        for (int c = 0; c < kRaggedClasses; c++) {
            const int th = kRaggedTh[c], tw = 4096 / th;
            for (int y = 0; y < area[c][1]; y += th)
                for (int x = 0; x < area[c][3]; x += tw)
                    plan->recs[c].push_back(
                        JbfTileRec{first, h, w, area[c][0] + y, area[c][2] + x, {0, 0}});
        }
        first += (unsigned long long)h * w;
    }
}

// One tile class of a ragged call: every image's tiles of TH rows in one launch.
template <int SCN, int GREP, int CREP, int TLW, int TH>
int launch_tile64_ragged(const JbfTables &t, int nz, int crows, const uint8_t *joint,
                         const uint8_t *src, uint8_t *dst, const JbfTileRec *d_recs, size_t ntiles,
                         int jcn, int border, int flags, hipStream_t stream)
{
    if (ntiles == 0)
        return RF_OK;
    if (!launch_fits(ntiles, 1024))
        return fail(RF_E_UNSUPPORTED, "rf_jbf_ragged_u8: too many tiles for one launch");
    auto kern = jbf_tile64_kernel<SCN, GREP, CREP, TLW, TH, true>;
    RF_HIP_CHECK(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize,
                                     kT64Lds));
    hipLaunchKernelGGL(kern, dim3((unsigned)ntiles), dim3(1024), kT64Lds, stream, joint, src, dst, 0,
                       0, jcn, t.radius, border, t.d_lut, nz, t.d_hw, t.d_swsym, t.sw_len, d_recs, 0,
                       flags, crows, 0, 0, JbfNoTileFlags{});
    return RF_OK;
}

// The launches of a ragged plan; d_recs[c] = the device copy of plan.recs[c].
template <int SCN, int GREP, int CREP, int TLW>
int launch_ragged(const JbfTables &t, int nz, const RaggedPlan &plan, const uint8_t *joint,
                  const uint8_t *src, uint8_t *dst, const JbfTileRec *const *d_recs, int jcn,
                  int border, int flags, hipStream_t stream)
{
    int rc = launch_tile64_ragged<SCN, GREP, CREP, TLW, 64>(t, nz, plan.shape.crows, joint, src, dst,
                                                            d_recs[0], plan.recs[0].size(), jcn,
                                                            border, flags, stream);
    if constexpr (TLW == 144) {
        if (rc == RF_OK)
            rc = launch_tile64_ragged<SCN, GREP, CREP, 208, 32>(t, nz, 32, joint, src, dst, d_recs[1],
                                                                plan.recs[1].size(), jcn, border,
                                                                flags, stream);
        if constexpr (SCN == 1) {
            if (rc == RF_OK)
                rc = launch_tile64_ragged<1, GREP, CREP, 336, 16>(t, nz, 32, joint, src, dst,
                                                                  d_recs[2], plan.recs[2].size(), jcn,
                                                                  border, flags, stream);
            if (rc == RF_OK)
                rc = launch_tile64_ragged<1, GREP, CREP, 136, 128>(t, nz, 32, joint, src, dst,
                                                                   d_recs[3], plan.recs[3].size(),
                                                                   jcn, border, flags, stream);
        }
    }
    return rc;
}

// ------------------------------------------------------------------------------------------
// Radius 53..468 (--sigma_spatial is a free float of the reference's tool,
// /root/reference/filter_reflectance.py:117-119: sigma 36 -> radius 54, 47 -> 70, 66 -> 99, 88 -> 132):
// the 64x64 tile with its halo no longer fits the LDS.  The workgroup covers its 64x64 outputs in bands of
// `crows` rows (all 64 - every lane busy - wherever that leaves room for a slab of 24 rows) and takes
// the disk's 2r + 1 tap rows in SLABS of `slab_rows`: the LDS holds the band's rows plus one slab of
// halo at a time, 4-byte texels {B,G,R joint, ONE src byte}, the accumulators stay in registers from
// slab to slab (jbf_tap_loop_grey4_la2<.., SLAB>; the weights come through scalar loads, so the LDS
// holds only tile and LUT), and every pixel's taps still arrive in row-major order - the bytes of
// the one-pass kernels.  The row pitch (64 outputs + 2 r4 + 8 columns) is bounded by the 8-bit offsets
// of the loop's ds_read2: 1008 texels, r4 <= 468 (pitches in steps of 32 up to 336, coarser beyond: a
// wider pitch than needed only costs slab rows); beyond that the untiled kernel remains.  A 3-channel
// src whose channels differ takes ONE pass of the colour loop on 6-byte texels
// (jbf_tap_loop_rgb6<.., SLAB>; one pass per channel of the grey loop only where the second plane
// leaves no room for a slab); a scan of the tile's src bytes up front sends a grey 3-channel tile to
// the grey loop.  Round 5's row-band kernel (radius 53..72: bands of 32 / 16 / 8 rows with the
// whole halo staged, i.e. a half to an eighth of the lanes busy) is gone: slabs run 7.3 G taps/s at
// every radius (0.95 of the radius-33 rate) where the bands ran 6.7 at radius 54, 3.7 at radius 70.
// ------------------------------------------------------------------------------------------
// kRagged (rf_jbf_ragged_u8): the workgroup's image, size and tile origin come from its 32-byte
// record, as in jbf_tile64_kernel; bands, slabs and pitch depend on the tables only and stay per launch.
template <int GREP, int TLW, bool kRagged = false>
__global__ __launch_bounds__(1024) void jbf_slab_kernel(
    const uint8_t *__restrict__ joint, const uint8_t *__restrict__ src, uint8_t *__restrict__ dst,
    int h, int w, int jcn, int scn, int radius, int border, const float *__restrict__ lut, int nz,
    const int *__restrict__ hwtab, const float *__restrict__ swsym, int sw_len,
    typename JbfTilesArg<kRagged>::type tiles_x, int tiles_per_img, int flags, int crows_g, int slab_g,
    int crows_c, int slab_c)
{
    // crows_g / slab_g: rows per band and per slab with 4-byte texels (grey src, or a 3-channel src
    // whose tile turns out grey); crows_c / slab_c with 6-byte texels (colour src, one pass: main
    // plane {B,G,R joint, B src} + a plane of 2-byte texels {G src, R src}, jbf_tap_loop_rgb6);
    // crows_c = 0: no room for the second plane - one grey pass per channel
    constexpr int NT = 1024, Q4 = TLW / 4, QW = 16;
    static_assert(TLW % 32 == 16, "row pitch keeps the rows of a half-wave on disjoint banks");
    extern __shared__ __align__(16) unsigned char smem[];
    int *flag_word = reinterpret_cast<int *>(smem);
    uint32_t *tile4 = reinterpret_cast<uint32_t *>(smem + 16);
    const int tid = threadIdx.x;
    if (tid == 0)
        *flag_word = 3;
    const int tile_id = xcd_contiguous_tile((int)blockIdx.x, (int)gridDim.x);
    int tile_y0, tile_x0;
    size_t img;
    if constexpr (kRagged) {
        // one record per workgroup: the same words in every lane (scalar loads, scalar registers) -
        // h and the tile's origin bound the band and slab loops, whose bounds are scalar-load addresses
        const JbfTileRec *rec = tiles_x + tile_id;
        img = (size_t)rec->first;
        h = rec->h;
        w = rec->w;
        tile_y0 = rec->tile_y0;
        tile_x0 = rec->tile_x0;
    } else {
        const int img_idx = tile_id / tiles_per_img;
        const int t_in_img = tile_id - img_idx * tiles_per_img;
        tile_y0 = (t_in_img / tiles_x) * 64;
        tile_x0 = (t_in_img % tiles_x) * 64;
        img = (size_t)img_idx * h * w;
    }
    const int r4 = (radius + 3) & ~3;
    const int tx = tid % QW, ty = tid / QW;
    float *lut_g = reinterpret_cast<float *>(smem + kT64Lds - nz * GREP * 4);
    for (int i = tid; i < nz * GREP; i += NT)
        lut_g[i] = lut[i / GREP];
    const uint32_t lut_lane_addr = lds_addr(lut_g) + (uint32_t)(tid & (GREP - 1)) * 4u;
    const uint32_t tile_lane_addr = lds_addr(tile4) + (uint32_t)tx * 4u;
    // 3-channel src: is every src texel the tile's 64 rows will ever stage grey (B = G = R)?  One scan
    // of the src bytes of tile + halo up front (a texel is then used by thousands of taps): a grey tile
    // - the reference filters the CNN's grey map as a 3-channel image - takes ONE pass of the grey loop
    int all_grey = scn == 1;
    if (scn == 3) {
        int grey = 1;
        const int rows_all = min(64, h - tile_y0) + 2 * radius;
        for (int item = tid; item < rows_all * Q4; item += NT) {
            const int ry = item / Q4, k = item - ry * Q4;
            const int gy = border_interpolate(tile_y0 - radius + ry, h, border);
            uint32_t jv[4], sv[4];
            load_tile_quad(joint, src, img, gy, tile_x0 - r4 + 4 * k, w, jcn, scn, border, jv, sv);
#pragma unroll
            for (int u = 0; u < 4; u++)
                grey &= (int)(((sv[u] ^ (sv[u] >> 8)) & 0xffffu) == 0u);
        }
        // (the same word in every lane; said so, or the slab bounds - scalar-load addresses - count as divergent)
        all_grey = __builtin_amdgcn_readfirstlane(block_all2(grey, 1, flag_word) & 1);  // (barrier inside)
    }
    const bool rgb6 = !all_grey && crows_c > 0;
    const int crows = rgb6 ? crows_c : crows_g, slab_rows = rgb6 ? slab_c : slab_g;
    const bool active = tid < QW * crows;
    for (int y0 = tile_y0; y0 < tile_y0 + 64 && y0 < h; y0 += crows) {
        for (int c = 0; c < (all_grey || rgb6 ? 1 : scn); c++) {
            // the lane's four centre pixels (their joint values; border arithmetic as in the tile)
            uint32_t jc[kPix];
            float sum1[kPix][1], sum3[kPix][3], wsum[kPix];
            {
                uint32_t jv[4], sv[4];
                load_tile_quad(joint, src, img, min(y0 + ty, h - 1), tile_x0 + 4 * tx, w, jcn, scn, border,
                               jv, sv);
#pragma unroll
                for (int p = 0; p < kPix; p++) {
                    jc[p] = jv[p] & 0x00ffffffu;
                    sum1[p][0] = sum3[p][0] = sum3[p][1] = sum3[p][2] = 0.f;
                    wsum[p] = 0.f;
                }
            }
            // per wave, for all its slabs: the masked-SAD form of the loops unless a centre has a zero channel
            const bool msad = !(flags & kJbfNoMsad) && jbf_wave_takes_msad(jc, active);
            for (int i0 = -radius; i0 <= radius; i0 += slab_rows) {
                const int i1 = min(i0 + slab_rows - 1, radius);
                const int tlh = crows + (i1 - i0);
                uint16_t *plane_b = reinterpret_cast<uint16_t *>(tile4 + (size_t)tlh * TLW);
                __syncthreads();  // everyone is done with the previous contents of the tile
                for (int item = tid; item < tlh * Q4; item += NT) {
                    const int ry = item / Q4, k = item - ry * Q4;
                    const int gy = border_interpolate(y0 + i0 + ry, h, border);
                    uint32_t jv[4], sv[4];
                    load_tile_quad(joint, src, img, gy, tile_x0 - r4 + 4 * k, w, jcn, scn, border, jv, sv);
#pragma unroll
                    for (int u = 0; u < 4; u++) {
                        tile4[ry * TLW + u * Q4 + k] = jv[u] | (((sv[u] >> (8 * c)) & 0xffu) << 24);
                        if (rgb6)
                            plane_b[ry * TLW + u * Q4 + k] = (uint16_t)(sv[u] >> 8);
                    }
                }
                __syncthreads();
                if (active) {
                    if (rgb6 && msad)
                        jbf_tap_loop_rgb6<GREP, TLW, true, true>(lut_lane_addr, swsym, tile_lane_addr,
                                                                 lds_addr(plane_b) + (uint32_t)tx * 2u, jc, ty,
                                                                 radius, r4, sw_len, hwtab, sum3, wsum, i0, i1,
                                                                 -i0);
                    else if (rgb6)
                        jbf_tap_loop_rgb6<GREP, TLW, true>(lut_lane_addr, swsym, tile_lane_addr,
                                                           lds_addr(plane_b) + (uint32_t)tx * 2u, jc, ty,
                                                           radius, r4, sw_len, hwtab, sum3, wsum, i0, i1, -i0);
                    else if (msad)
                        jbf_tap_loop_grey4_la2<GREP, TLW, false, true, true>(lut_lane_addr, swsym,
                                                                             tile_lane_addr, jc, ty, radius, r4,
                                                                             sw_len, hwtab, sum1, wsum, i0, i1,
                                                                             -i0);
                    else
                        jbf_tap_loop_grey4_la2<GREP, TLW, false, true>(lut_lane_addr, swsym, tile_lane_addr,
                                                                       jc, ty, radius, r4, sw_len, hwtab,
                                                                       sum1, wsum, i0, i1, -i0);
                }
            }
            if (active) {
                if (rgb6)
                    store_quad<3, 3>(dst, img, y0 + ty, tile_x0 + 4 * tx, h, w, sum3, wsum, flags);
                else if (scn == 1)
                    store_quad<1, 1>(dst, img, y0 + ty, tile_x0 + 4 * tx, h, w, sum1, wsum, flags);
                else if (all_grey)
                    store_quad<1, 3>(dst, img, y0 + ty, tile_x0 + 4 * tx, h, w, sum1, wsum, flags);
                else
                    store_quad_channel(dst, img, y0 + ty, tile_x0 + 4 * tx, h, w, c, sum1, wsum, flags);
            }
        }
    }
}

// rows per band and per slab of jbf_slab_kernel at row pitch tlw for a LUT replicated grep times
// (crows = 0: does not fit): all 64 rows of the tile in one band - every lane busy - as long as a
// slab is at least 24 rows, else 32, else 16
// (texel_bytes: 4 for the grey-packed plane alone, 6 with the colour plane beside it)
void slab_fits(const JbfTables &t, int nz, int grep, int tlw, int texel_bytes, int *crows, int *slab_rows)
{
    *crows = *slab_rows = 0;
    if (2 * t.r4 + 64 + 8 > tlw)
        return;
    const long long rows =
        ((long long)kT64Lds - 16 - (long long)nz * grep * 4) / ((long long)tlw * texel_bytes);
    for (int cr : {64, 32, 16}) {
        const long long sl = rows - cr + 1;
        if (sl >= (cr == 16 ? 8 : 24)) {
            *crows = cr;
            *slab_rows = (int)std::min<long long>(sl, 2 * t.radius + 1);
            return;
        }
    }
}

// The row pitches jbf_slab_kernel is instantiated for, narrowest first: X(largest r4 served, pitch).
// Steps of 32 up to 336, coarser beyond (a wider pitch than needed only costs slab rows).
#define RF_SLAB_PITCHES(X)                                                                    \
    X(68, 208) X(84, 240) X(100, 272) X(116, 304) X(132, 336) X(164, 400) X(212, 496) X(276, 624) \
    X(372, 816) X(kJbfMaxTiledR4, 1008)

// The shape a call of radius 53..468 runs at; it depends on the tables, not on the image sizes.
// The narrowest pitch that holds r4; 16 LUT replicas unless 8 leave a taller band; a colour src
// takes the 6-byte rows that fit beside the same replicas.  False: outside the radii, or nothing fits.
bool slab_choose(const JbfTables &t, int nz, int src_cn, SlabShape *out)
{
    if (t.r4 <= 52 || t.r4 > kJbfMaxTiledR4)
        return false;
    SlabShape s{};
#define RF_PITCH(R4_, TLW_) \
    if (!s.tlw && t.r4 <= R4_) \
        s.tlw = TLW_;
    RF_SLAB_PITCHES(RF_PITCH)
#undef RF_PITCH
    for (int g : {16, 8}) {
        int cr, sl;
        slab_fits(t, nz, g, s.tlw, 4, &cr, &sl);
        if (cr > s.crows_g)
            s.crows_g = cr, s.slab_g = sl, s.grep = g;
    }
    if (s.crows_g == 0)
        return false;
    if (src_cn == 3)  // a colour tile in one pass: 6-byte texels, same replicas
        slab_fits(t, nz, s.grep, s.tlw, 6, &s.crows_c, &s.slab_c);
    *out = s;
    return true;
}

template <int GREP, int TLW>
int launch_slab(const JbfTables &t, int nz, int crows, int slab_rows, int crows_c, int slab_c,
                const uint8_t *joint, const uint8_t *src, uint8_t *dst, int n, int h, int w, int jcn,
                int scn, int border, int flags, hipStream_t stream)
{
    const int tiles_x = ceil_div(w, 64), tiles_y = ceil_div(h, 64);
    const long long blocks = (long long)tiles_x * tiles_y * n;
    if (!launch_fits(blocks, 1024))
        return fail(RF_E_UNSUPPORTED, "rf_jbf_u8: batch too large for one launch");
    auto kern = jbf_slab_kernel<GREP, TLW>;
    RF_HIP_CHECK(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize,
                                     kT64Lds));
    hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(1024), kT64Lds, stream, joint, src, dst, h,
                       w, jcn, scn, t.radius, border, t.d_lut, nz, t.d_hw, t.d_swsym, t.sw_len,
                       tiles_x, tiles_x * tiles_y, flags, crows, slab_rows, crows_c, slab_c);
    return RF_OK;
}

// A ragged call at these radii: every image's 64x64 tiles in one launch.
template <int GREP, int TLW>
int launch_slab_ragged(const JbfTables &t, int nz, const SlabShape &s, const uint8_t *joint,
                       const uint8_t *src, uint8_t *dst, const JbfTileRec *d_recs, size_t ntiles,
                       int jcn, int scn, int border, int flags, hipStream_t stream)
{
    if (ntiles == 0)
        return RF_OK;
    if (!launch_fits(ntiles, 1024))
        return fail(RF_E_UNSUPPORTED, "rf_jbf_ragged_u8: too many tiles for one launch");
    auto kern = jbf_slab_kernel<GREP, TLW, true>;
    RF_HIP_CHECK(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize,
                                     kT64Lds));
    hipLaunchKernelGGL(kern, dim3((unsigned)ntiles), dim3(1024), kT64Lds, stream, joint, src, dst, 0,
                       0, jcn, scn, t.radius, border, t.d_lut, nz, t.d_hw, t.d_swsym, t.sw_len,
                       d_recs, 0, flags, s.crows_g, s.slab_g, s.crows_c, s.slab_c);
    return RF_OK;
}

// ------------------------------------------------------------------------------------------
// Two workgroups per CU (radius <= 36, pitch 144, 32 LUT replicas): the grey tiles of a call - a
// single-channel src, or a 3-channel src whose tile and halo are grey, the metric's case - in
// workgroups of 81,920 B of LDS and at most 64 VGPRs, so that a CU holds two of them: 8 waves per SIMD
// in the tap loop, and one workgroup's staging, vote and stores behind the other's loop.  The kernel
// holds the grey loop only.  The LUT sits at the end of the allocation (reads beyond it return 0:
// lds_oob_probe_half_kernel), the rows in front of it hold 64 output rows plus a slab of the disk's tap
// rows, walked as in jbf_slab_kernel: same loop (SLAB), accumulators in registers from slab to slab,
// every pixel's taps in row-major order - the bytes of jbf_tile64_kernel.  What jbf_tile64_kernel votes on
// (are the texels of tile and halo grey?) is one byte per tile in tile_flags here, written first: by the
// grey map (jbf_grey_map_kernel, rf_jbf_greymap.hip: one pass over the images, in front of it the launch that
// clears the bytes), or under "jbf_vote_scan" by a launch of this kernel of its own (kJbfVoteOnly) in which every tile
// scans its region; a grey joint is then staged in the J1 form at once.  A tile whose src is not grey is
// not filtered here: a launch of jbf_tile64_kernel<.., kFlagged> over the same grid filters exactly
// those tiles, and the filtering launch of this kernel leaves them after one scalar load.  The launches
// then - clear, grey map, flagged colour tiles (3-channel src only), grey tiles, in this order: for a grey
// batch the last one does the work.  Single-channel buffers need no bytes (one launch).
// ------------------------------------------------------------------------------------------
// rows of the tile in front of the LUT, and the tap rows of a slab (0: no room)
int tile64x2_slab_rows(int nz, int grep, int tlw)
{
    // (nothing beside tile and LUT: at sigma_color 20 the LUT's 289 entries leave exactly 78 rows of pitch 144)
    const int rows = (kT64x2Lds - nz * grep * 4) / (tlw * 4);
    return rows >= 64 ? rows - 64 + 1 : 0;
}

// (the second launch bound is waves per SIMD: two workgroups of 16 waves on a CU's four SIMDs)
template <int GREP, int TLW>
__global__ __launch_bounds__(1024, 8) void jbf_tile64x2_kernel(
    const uint8_t *__restrict__ joint, const uint8_t *__restrict__ src, uint8_t *__restrict__ dst,
    int h, int w, int jcn, int scn, int radius, int border, const float *__restrict__ lut, int nz,
    const int *__restrict__ hwtab, const float *__restrict__ swsym, int sw_len, int tiles_x,
    int tiles_per_img, int flags, int slab_rows, uint8_t *__restrict__ tile_flags)
{
    constexpr int NT = 1024, Q4 = TLW / 4, QW = 16;
    static_assert(TLW % 32 == 16, "row pitch keeps the rows of a half-wave on disjoint banks");
    extern __shared__ __align__(16) unsigned char smem[];
    // the vote's word lies in the tile's first texel: the vote is over (every lane has read the word) before
    // the barrier in front of the first staging
    int *flag_word = reinterpret_cast<int *>(smem);
    uint32_t *tile4 = reinterpret_cast<uint32_t *>(smem);
    const int tid = threadIdx.x;
    if (tid == 0)
        *flag_word = 3;
    __syncthreads();
    const int tile_id = xcd_contiguous_tile((int)blockIdx.x, (int)gridDim.x);
    const int img_idx = tile_id / tiles_per_img;
    const int t_in_img = tile_id - img_idx * tiles_per_img;
    const int tile_y0 = (t_in_img / tiles_x) * 64;
    const int tile_x0 = (t_in_img % tiles_x) * 64;
    const size_t img = (size_t)img_idx * h * w;
    const int r4 = (radius + 3) & ~3;
    const int tx = tid % QW, ty = tid / QW;
    // the vote of jbf_tile64_kernel, in a launch of its own (kJbfVoteOnly) in front of the filtering ones: is
    // every src texel of tile and halo grey (B = G = R), and every joint texel?  The tile's byte: bit 0 = the
    // src is NOT grey, bit 1 = the joint is.  (1-channel buffers need no look: no vote launch, no bytes.)
    int grey_joint = 1;
    if (flags & kJbfVoteOnly) {
        int grey = 1;
        const int rows_all = 64 + 2 * radius;
        for (int item = tid; item < rows_all * Q4; item += NT) {
            const int ry = item / Q4, k = item - ry * Q4;
            const int gy = border_interpolate(tile_y0 - radius + ry, h, border);
            uint32_t jv[4], sv[4];
            load_tile_quad(joint, src, img, gy, tile_x0 - r4 + 4 * k, w, jcn, scn, border, jv, sv);
#pragma unroll
            for (int u = 0; u < 4; u++) {
                if (scn == 3)
                    grey &= (int)(((sv[u] ^ (sv[u] >> 8)) & 0xffffu) == 0u);
                if (jcn == 3)
                    grey_joint &= (int)(((jv[u] ^ (jv[u] >> 8)) & 0xffffu) == 0u);
            }
        }
        // (the same word in every lane; said so, or the slab bounds - scalar-load addresses - count as divergent)
        const int bits = block_all2(grey, grey_joint, flag_word);  // (barrier inside)
        if (tid == 0)
            tile_flags[tile_id] = (uint8_t)(((bits & 1) ? 0 : 1) | (bits & 2));
        return;
    }
    if (tile_flags) {
        // (one scalar load; the same byte in every lane - the slab bounds below are scalar-load addresses)
        const int byte = __builtin_amdgcn_readfirstlane((int)tile_flags[tile_id]);
        if (byte & 1)
            return;  // a colour tile: jbf_tile64_kernel<.., kFlagged> filters it
        grey_joint = (byte >> 1) & 1;
    }
    float *lut_g = reinterpret_cast<float *>(smem + kT64x2Lds - nz * GREP * 4);
    for (int i = tid; i < nz * GREP; i += NT)
        lut_g[i] = lut[i / GREP];
    const uint32_t lut_lane_addr = lds_addr(lut_g) + (uint32_t)(tid & (GREP - 1)) * 4u;
    const uint32_t tile_lane_addr = lds_addr(tile4) + (uint32_t)tx * 4u;
    // grey src and grey joint: the joint field of a texel holds the value times the LUT's byte stride
    // (jbf_tile64_kernel's j1 / j1_late), which turns the SAD of the tap loop into the gather address
    const bool j1 = grey_joint != 0;
    const uint32_t j1_scale = (uint32_t)(jcn == 1 ? 1 : 3) * (GREP * 4u);
    // the lane's four centre pixels (their joint values; border arithmetic as in the tile)
    uint32_t jc[kPix];
    float sum1[kPix][1], wsum[kPix];
    {
        uint32_t jv[4], sv[4];
        load_tile_quad(joint, src, img, border_interpolate(tile_y0 + ty, h, border), tile_x0 + 4 * tx, w, jcn,
                       scn, border, jv, sv);
#pragma unroll
        for (int p = 0; p < kPix; p++) {
            jc[p] = j1 ? (jv[p] & 0xffu) * j1_scale : jv[p] & 0x00ffffffu;
            sum1[p][0] = 0.f;
            wsum[p] = 0.f;
        }
    }
    // per wave, for all its slabs: the masked-SAD form of the loop unless a centre has a zero channel
    const bool msad = !j1 && !(flags & kJbfNoMsad) && jbf_wave_takes_msad(jc);
    // a wave whose four tile rows all lie below the image (at 1080 rows two of sixteen in the last row of
    // tiles) has nothing to store: it stages and meets every barrier, and walks no taps.  (Per wave and by rows
    // only: a tile that overhangs the image's right edge - any width that is no multiple of 64 - has dead
    // lanes in every wave, never a dead wave.)
    const bool live_wave =
        __builtin_amdgcn_readfirstlane(tile_y0 + (ty & ~3)) < h || (flags & kJbfNoDeadSkip) != 0;
    for (int i0 = -radius; i0 <= radius; i0 += slab_rows) {
        const int i1 = min(i0 + slab_rows - 1, radius);
        const int tlh = 64 + (i1 - i0);
        __syncthreads();  // everyone is done with the previous contents of the tile
        for (int item = tid; item < tlh * Q4; item += NT) {
            const int ry = item / Q4, k = item - ry * Q4;
            const int gy = border_interpolate(tile_y0 + i0 + ry, h, border);
            uint32_t jv[4], sv[4];
            load_tile_quad(joint, src, img, gy, tile_x0 - r4 + 4 * k, w, jcn, scn, border, jv, sv);
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const uint32_t jfield = j1 ? (jv[u] & 0xffu) * j1_scale : jv[u];
                tile4[ry * TLW + u * Q4 + k] = jfield | (sv[u] << 24);
            }
        }
        __syncthreads();
        if (!live_wave)
            continue;
        if (j1)
            jbf_tap_loop_grey4_la2<GREP, TLW, true, true>(lut_lane_addr, swsym, tile_lane_addr, jc, ty,
                                                          radius, r4, sw_len, hwtab, sum1, wsum, i0, i1, -i0);
        else if (msad)
            jbf_tap_loop_grey4_la2<GREP, TLW, false, true, true>(lut_lane_addr, swsym, tile_lane_addr, jc,
                                                                 ty, radius, r4, sw_len, hwtab, sum1, wsum,
                                                                 i0, i1, -i0);
        else
            jbf_tap_loop_grey4_la2<GREP, TLW, false, true>(lut_lane_addr, swsym, tile_lane_addr, jc, ty,
                                                           radius, r4, sw_len, hwtab, sum1, wsum, i0, i1,
                                                           -i0);
    }
    if (scn == 1)
        store_quad<1, 1>(dst, img, tile_y0 + ty, tile_x0 + 4 * tx, h, w, sum1, wsum, flags);
    else
        store_quad<1, 3>(dst, img, tile_y0 + ty, tile_x0 + 4 * tx, h, w, sum1, wsum, flags);
}

// The flag bytes of the two-launch route: one library-owned buffer per (device, stream), kept from
// call to call and enlarged only outside a stream capture.  An outgrown buffer is kept until
// rf_jbf_release_scratch / rf_shutdown: a captured graph may still name it.
struct TileFlagBuf {
    int dev;
    hipStream_t stream;
    uint8_t *p;
    size_t bytes;
};
std::mutex g_tf_mu;
std::vector<TileFlagBuf> g_tf;        // (guarded by g_tf_mu)
std::vector<uint8_t *> g_tf_retired;  // (guarded by g_tf_mu)
constexpr size_t kTileFlagStreams = 16;  // (device, stream) pairs that hold a buffer; further ones take the old path
std::atomic<int> g_two_wg_calls{0};      // calls that launched the route (rf_debug_jbf_two_wg_calls)

// bytes of the buffer that serves a launch of `tiles` tiles: the power of two >= tiles, 4 KiB at least
size_t tile_flag_bytes(size_t tiles)
{
    size_t b = 4096;
    while (b < tiles)
        b <<= 1;
    return b;
}

// *out = nullptr: no buffer of that size and none may be made now (the stream is capturing, or
// kTileFlagStreams other streams hold one)
int get_tile_flags(int dev, hipStream_t stream, size_t tiles, uint8_t **out)
{
    *out = nullptr;
    std::lock_guard<std::mutex> lock(g_tf_mu);
    size_t at = g_tf.size();
    for (size_t i = 0; i < g_tf.size(); i++)
        if (g_tf[i].dev == dev && g_tf[i].stream == stream)
            at = i;
    if (at < g_tf.size() && g_tf[at].bytes >= tiles) {
        *out = g_tf[at].p;
        return RF_OK;
    }
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(stream, &st) != hipSuccess || st != hipStreamCaptureStatusNone) {
        (void)hipGetLastError();
        return RF_OK;
    }
    // a stream beyond the kTileFlagStreams that hold a buffer gets none (no buffer is taken from a stream: a
    // captured graph may name it), so what the library holds is bounded: per stream the sizes it grew through
    if (at == g_tf.size() && g_tf.size() >= kTileFlagStreams)
        return RF_OK;
    uint8_t *p = nullptr;
    {
        CaptureRelax relax;  // (another thread of the process may be capturing in the global mode)
        RF_HIP_CHECK(hipMalloc(&p, tile_flag_bytes(tiles)));
    }
    if (at < g_tf.size()) {
        g_tf_retired.push_back(g_tf[at].p);
        g_tf.erase(g_tf.begin() + at);
    }
    g_tf.push_back(TileFlagBuf{dev, stream, p, tile_flag_bytes(tiles)});
    *out = p;
    return RF_OK;
}

// Does a call take the two-workgroups-per-CU route?  Decided from the tables and the flags alone.
// *slab_rows: tap rows per slab (the tile holds 64 + slab_rows - 1 rows).
bool two_wg_choose(const JbfTables &t, int nz, int src_cn, int flags, int *slab_rows)
{
    *slab_rows = 0;
    if (debug_get(kDbgJbfNoTwoWg) || debug_get(kDbgJbfTune) ||
        (flags & (RF_JBF_FORCE_GENERIC | kJbfStageOnly | kJbfCompilerLoop | kJbfLookahead1)))
        return false;
    Tile64Shape shape;
    if (t.r4 > 36 || !tile64_choose(t, nz, src_cn, flags, &shape) || shape.tlw != 144 || shape.grep != 32)
        return false;
    *slab_rows = tile64x2_slab_rows(nz, 32, 144);
    return *slab_rows >= 8;
}

// The 64x64 tiles of the main area [0, rows) x [0, cols) of every image: with kJbfVoteOnly in flags the
// launch that writes their vote bytes, without it the launch that filters the grey ones (tile_flags may
// be NULL then: single-channel buffers, every tile grey).
int launch_tile64x2(const JbfTables &t, int nz, int slab_rows, const uint8_t *joint, const uint8_t *src,
                    uint8_t *dst, int n, int h, int w, int jcn, int scn, int border, int flags,
                    hipStream_t stream, int rows, int cols, uint8_t *tile_flags)
{
    const int tiles_x = ceil_div(cols, 64), tiles_y = ceil_div(rows, 64);
    const long long blocks = (long long)tiles_x * tiles_y * n;
    auto kern = jbf_tile64x2_kernel<32, 144>;
    RF_HIP_CHECK(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize,
                                     kT64x2Lds));
    hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(1024), kT64x2Lds, stream, joint, src, dst, h, w,
                       jcn, scn, t.radius, border, t.d_lut, nz, t.d_hw, t.d_swsym, t.sw_len, tiles_x,
                       tiles_x * tiles_y, flags, slab_rows, tile_flags);
    return RF_OK;
}

template <int CREP>
int launch_tile64_flagged(const JbfTables &t, int nz, int crows, const uint8_t *joint, const uint8_t *src,
                          uint8_t *dst, int n, int h, int w, int jcn, int border, int flags,
                          hipStream_t stream, int rows, int cols, const uint8_t *tile_flags)
{
    const int tiles_x = ceil_div(cols, 64), tiles_y = ceil_div(rows, 64);
    const long long blocks = (long long)tiles_x * tiles_y * n;
    auto kern = jbf_tile64_kernel<3, 32, CREP, 144, 64, false, true>;
    RF_HIP_CHECK(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize,
                                     kT64Lds));
    hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(1024), kT64Lds, stream, joint, src, dst, h, w,
                       jcn, t.radius, border, t.d_lut, nz, t.d_hw, t.d_swsym, t.sw_len, tiles_x,
                       tiles_x * tiles_y, flags, crows, 0, 0, tile_flags);
    return RF_OK;
}

// A call on the two-per-CU route: the tile bytes (3-channel src or joint), the flagged tiles of a 3-channel src
// in jbf_tile64_kernel, the grey tiles in jbf_tile64x2_kernel, the strips as ever.  *done = false (nothing
// launched): no main area, or no flag buffer may be made now - the caller takes the one-per-CU path.
int launch_two_wg(const JbfTables &t, int nz, const Tile64Shape &shape, int slab_rows,
                  const uint8_t *joint, const uint8_t *src, uint8_t *dst, int n, int h, int w, int jcn,
                  int scn, int border, int flags, hipStream_t stream, bool *done)
{
    *done = false;
    const Tile64Areas a = tile64_areas(t, nz, shape.grep, shape.crep, scn, flags, h, w);
    if (a.rows_main <= 0 || a.cols_main <= 0)
        return RF_OK;
    const long long blocks = (long long)ceil_div(a.cols_main, 64) * ceil_div(a.rows_main, 64) * n;
    if (!launch_fits(blocks, 1024))
        return fail(RF_E_UNSUPPORTED, "rf_jbf_u8: batch too large for one launch");
    // launch order: the tile bytes (cleared, then the grey map's pass over the images), the flagged colour
    // tiles, the grey tiles - the launch that does a grey batch's work comes last (a profile that takes a
    // call's last launch for the call reads the metric kernel)
    uint8_t *tile_flags = nullptr;
    int rc = RF_OK;
    if (scn == 3 || jcn == 3) {
        if (int bad = get_tile_flags(t.device, stream, (size_t)blocks, &tile_flags))
            return bad;
        if (!tile_flags)
            return RF_OK;
        const int tiles_x = ceil_div(a.cols_main, 64), tiles_y = ceil_div(a.rows_main, 64);
        // "jbf_vote_scan", a WRAP border or a region the map's blocks do not reach: every tile scans its region
        if (debug_get(kDbgJbfVoteScan) || !jbf_grey_map_serves(h, w, t.radius, border, tiles_x, tiles_y))
            rc = launch_tile64x2(t, nz, slab_rows, joint, src, dst, n, h, w, jcn, scn, border,
                                 flags | kJbfVoteOnly, stream, a.rows_main, a.cols_main, tile_flags);
        else
            rc = jbf_launch_grey_map(joint, src, n, h, w, jcn, scn, t.radius, border, stream, tiles_x, tiles_y,
                                     tile_flags);
    }
    if (rc == RF_OK && scn == 3)
        rc = shape.crep == 32 ? launch_tile64_flagged<32>(t, nz, shape.crows, joint, src, dst, n, h, w, jcn,
                                                          border, flags, stream, a.rows_main, a.cols_main,
                                                          tile_flags)
                              : launch_tile64_flagged<16>(t, nz, shape.crows, joint, src, dst, n, h, w, jcn,
                                                          border, flags, stream, a.rows_main, a.cols_main,
                                                          tile_flags);
    if (rc == RF_OK)
        rc = launch_tile64x2(t, nz, slab_rows, joint, src, dst, n, h, w, jcn, scn, border, flags, stream,
                             a.rows_main, a.cols_main, tile_flags);
    if (rc == RF_OK && (a.s32 || a.s16 || a.sx)) {
        if (scn == 3)
            rc = shape.crep == 32 ? launch_tile64_rows<3, 32, 32>(t, nz, shape.crows, joint, src, dst, n, h, w,
                                                                  jcn, border, flags, stream, true)
                                  : launch_tile64_rows<3, 32, 16>(t, nz, shape.crows, joint, src, dst, n, h, w,
                                                                  jcn, border, flags, stream, true);
        else
            rc = shape.crep == 32 ? launch_tile64_rows<1, 32, 32>(t, nz, shape.crows, joint, src, dst, n, h, w,
                                                                  jcn, border, flags, stream, true)
                                  : launch_tile64_rows<1, 32, 16>(t, nz, shape.crows, joint, src, dst, n, h, w,
                                                                  jcn, border, flags, stream, true);
    }
    *done = rc == RF_OK;
    if (*done)
        g_two_wg_calls.fetch_add(1, std::memory_order_relaxed);
    return rc;
}

}  // namespace

void jbf_scratch_release()
{
    std::lock_guard<std::mutex> lock(g_tf_mu);
    for (const TileFlagBuf &b : g_tf)
        (void)hipFree(b.p);
    for (uint8_t *p : g_tf_retired)
        (void)hipFree(p);
    g_tf.clear();
    g_tf_retired.clear();
}

}  // namespace rf

extern "C" int rf_debug_jbf_two_wg_calls(void)
{
    return rf::g_two_wg_calls.load(std::memory_order_relaxed) & 0x7fffffff;
}

extern "C" int rf_debug_jbf_tile_flags(void *stream_, unsigned char *out, int cap)
{
    using namespace rf;
    hipStream_t stream = (hipStream_t)stream_;
    if (cap < 0 || (!out && cap))
        return fail(RF_E_BADARG, "rf_debug_jbf_tile_flags: NULL out or a negative cap");
    if (stream_is_capturing(stream))
        return fail(RF_E_UNSUPPORTED, "rf_debug_jbf_tile_flags: synchronises its stream and cannot be "
                                      "captured into a graph");
    int dev = 0;
    RF_HIP_CHECK(hipGetDevice(&dev));
    const uint8_t *p = nullptr;
    size_t bytes = 0;
    {
        std::lock_guard<std::mutex> lock(g_tf_mu);
        for (const TileFlagBuf &b : g_tf)
            if (b.dev == dev && b.stream == stream)
                p = b.p, bytes = b.bytes;
    }
    if (bytes > (size_t)cap)
        bytes = (size_t)cap;
    if (bytes) {
        RF_HIP_CHECK(hipMemcpyAsync(out, p, bytes, hipMemcpyDeviceToHost, stream));
        RF_HIP_CHECK(hipStreamSynchronize(stream));
    }
    return (int)bytes;
}

extern "C" int rf_jbf_release_scratch(void)
{
    rf::jbf_scratch_release();
    return RF_OK;
}

extern "C" int rf_jbf_u8(const uint8_t *joint, const uint8_t *src, uint8_t *dst, int n, int h,
                         int w, int joint_cn, int src_cn, int d, double sigma_color,
                         double sigma_space, int border, int flags, void *stream_)
{
    using namespace rf;
    if (n == 0)  // an empty batch is valid whatever the (possibly NULL) pointers are
        return RF_OK;
    if (!joint || !src || !dst)
        return fail(RF_E_BADARG, "rf_jbf_u8: NULL image pointer");
    if (n < 0 || h <= 0 || w <= 0)
        return fail(RF_E_BADARG, "rf_jbf_u8: bad size n=%d h=%d w=%d", n, h, w);
    if (int bad = jbf_check_format("rf_jbf_u8", joint_cn, src_cn, border))
        return bad;
    {
        const size_t px = (size_t)n * h * w;
        if (ranges_overlap(dst, px * src_cn, joint, px * joint_cn) ||
            ranges_overlap(dst, px * src_cn, src, px * src_cn))
            return fail(RF_E_BADARG, "rf_jbf_u8: dst must not overlap an input");
    }
    if (flags & ~kJbfPublicFlags)
        return fail(RF_E_BADARG, "rf_jbf_u8: unknown flag bits 0x%x", flags);
    flags |= jbf_debug_flags();
    // OpenCV's sigma and radius rules, RF_JBF_GREY_AS_BGR: rf_jbf_common.hpp
    sigma_color = jbf_sigma(sigma_color);
    sigma_space = jbf_sigma(sigma_space);
    const int radius = jbf_radius(d, sigma_space);
    if (radius > kJbfMaxRadius)
        return fail(RF_E_UNSUPPORTED, "rf_jbf_u8: radius %d too large", radius);
    hipStream_t stream = (hipStream_t)stream_;
    const int jcn_kernel = jbf_kernel_cn(joint_cn, flags);
    joint_cn = jbf_table_cn(joint_cn, flags);
    JbfTables t;
    TablesHold hold{t};
    int rc = get_tables(radius, joint_cn, sigma_color, sigma_space, stream, &t);
    if (rc != RF_OK)
        return rc;

    // ---- kernel selection -------------------------------------------------------------
    // tune = 0: automatic; 1..6 force a (tile height, LUT replicas, full LUT) configuration of
    // the tiled kernel (benchmark aid, tools/jbf_tune.py).
    const int tune = debug_get(kDbgJbfTune) & 0xf;
    static const Tiled2Config kCfg[] = {{48, 16, false}, {32, 8, true},  {32, 32, false},
                                        {32, 16, false}, {64, 16, false}, {48, 8, false}};
    constexpr int kNumCfg = (int)(sizeof(kCfg) / sizeof(kCfg[0]));
    // measured on MI355X at 1080p: 3 waves/SIMD with a 16x replicated, clamped LUT wins for grey
    // src; the clamp-free 8x table is next
    // tune 7 forces the 64x64 kernel, tune 1..6 the 64xTH kernel
    bool done = false;
    if (!(flags & RF_JBF_FORCE_GENERIC) && t.r4 <= kJbfMaxTiledR4 && (tune == 0 || tune == 7)) {
        bool oob_ok = false, oob_half = false;
        rc = lds_oob_reads_zero(t.device, &oob_ok, &oob_half);
        if (rc != RF_OK)
            return rc;
        // table entries before the zero tail (the whole table if it has none)
        const int nz = t.lut_len < 256 * joint_cn ? t.lut_len - 1 : t.lut_len;
        if (oob_ok) {
            Tile64Shape shape;
            if (tile64_choose(t, nz, src_cn, flags, &shape)) {
                // pitch 144 at 32 replicas: grey tiles at two workgroups per CU
                int slab2 = 0;
                if (oob_half && two_wg_choose(t, nz, src_cn, flags, &slab2)) {
                    rc = launch_two_wg(t, nz, shape, slab2, joint, src, dst, n, h, w, jcn_kernel, src_cn,
                                       border, flags, stream, &done);
                    if (rc != RF_OK)
                        return rc;
                }
#define RF_T64(G_, C_, W_)                                                                        \
    if (!done && shape.grep == G_ && shape.crep == C_ && shape.tlw == W_) {                       \
        if (W_ == 144)                                                                            \
            rc = src_cn == 3 ? launch_tile64_rows<3, G_, C_>(t, nz, shape.crows, joint, src, dst, \
                                                             n, h, w, jcn_kernel, border, flags,  \
                                                             stream)                              \
                             : launch_tile64_rows<1, G_, C_>(t, nz, shape.crows, joint, src, dst, \
                                                             n, h, w, jcn_kernel, border, flags,  \
                                                             stream);                             \
        else                                                                                      \
            rc = src_cn == 3 ? launch_tile64<3, G_, C_, W_>(t, nz, shape.crows, joint, src, dst,  \
                                                            n, h, w, jcn_kernel, border, flags,   \
                                                            stream)                               \
                             : launch_tile64<1, G_, C_, W_>(t, nz, shape.crows, joint, src, dst,  \
                                                            n, h, w, jcn_kernel, border, flags,   \
                                                            stream);                              \
    }
                RF_T64_SHAPES(RF_T64)
#undef RF_T64
                if (rc != RF_OK)
                    return rc;
                done = true;
            }
            // radius 53..468: tap-row slabs (jbf_slab_kernel) at the narrowest pitch that holds r4
            SlabShape slab;
            if (!done && slab_choose(t, nz, src_cn, &slab)) {
#define RF_SLAB(R4_, TLW_)                                                                        \
    if (slab.tlw == TLW_)                                                                         \
        rc = slab.grep == 16                                                                      \
                 ? launch_slab<16, TLW_>(t, nz, slab.crows_g, slab.slab_g, slab.crows_c,          \
                                         slab.slab_c, joint, src, dst, n, h, w, jcn_kernel,       \
                                         src_cn, border, flags, stream)                           \
                 : launch_slab<8, TLW_>(t, nz, slab.crows_g, slab.slab_g, slab.crows_c,           \
                                        slab.slab_c, joint, src, dst, n, h, w, jcn_kernel, src_cn, \
                                        border, flags, stream);
                RF_SLAB_PITCHES(RF_SLAB)
#undef RF_SLAB
                if (rc != RF_OK)
                    return rc;
                done = true;
            }
        }
    }
    int cfg = -1;
    if (!done && !(flags & RF_JBF_FORCE_GENERIC) && t.r4 <= 36 && tune != 7) {
        for (int ci = 0; ci < kNumCfg; ci++) {
            if (tune != 0 && tune != ci + 1)
                continue;
            const Tiled2Config &c = kCfg[ci];
            if (tiled2_lds_bytes(t, c.th, c.lutrep, c.full_lut) <= (size_t)kMaxLds) {
                cfg = ci;
                break;
            }
        }
    }
    if (cfg >= 0) {
#define RF_T2(TH_, REP_)                                                                        \
    rc = src_cn == 3 ? launch_tiled2<3, TH_, REP_>(t, kCfg[cfg].full_lut, joint, src, dst, n, h, \
                                                   w, jcn_kernel, border, flags, stream)        \
                     : launch_tiled2<1, TH_, REP_>(t, kCfg[cfg].full_lut, joint, src, dst, n, h, \
                                                   w, jcn_kernel, border, flags, stream)
        switch (cfg) {
        case 0: RF_T2(48, 16); break;
        case 1: RF_T2(32, 8); break;
        case 2: RF_T2(32, 32); break;
        case 3: RF_T2(32, 16); break;
        case 4: RF_T2(64, 16); break;
        default: RF_T2(48, 8); break;
        }
#undef RF_T2
        if (rc != RF_OK)
            return rc;
    } else if (!done) {
        dim3 grid(ceil_div(w, 64), ceil_div(h, 4), n);
        if (n > 65535)
            return fail(RF_E_UNSUPPORTED, "rf_jbf_u8: generic path supports n <= 65535");
        hipLaunchKernelGGL(jbf_generic_kernel, grid, dim3(256), 0, stream, joint, src, dst, h, w,
                           jcn_kernel, src_cn, border, t.d_lut, t.d_di, t.d_dj, t.d_sw, t.maxk,
                           flags);
    }
    RF_HIP_CHECK(hipGetLastError());
    return RF_OK;
}

// ------------------------------------------------------------------------------------------
// Ragged form: images of different sizes packed one after another, one launch per tile class
// over all images (radius <= 52), one launch of the slab kernel over all images' 64x64 tiles
// (radius 53..468), else rf_jbf_u8 once per image.
// ------------------------------------------------------------------------------------------
namespace rf {
namespace {

// The checks of both ragged entries and of the plan query that need no device: sizes, channels,
// flags, radius, the launch rule (launch_fits).  *px = pixels of all images, *tiles = their 64x64-tile
// count (no plan has more tiles: a strip is only taken where it saves workgroups).
int ragged_check(const char *who, int n, const int *heights, const int *widths, int joint_cn,
                 int src_cn, int d, double sigma_space, int border, int flags, size_t *px,
                 size_t *tiles)
{
    if (!heights || !widths)
        return fail(RF_E_BADARG, "%s: NULL size array", who);
    if (n < 0)
        return fail(RF_E_BADARG, "%s: bad size n=%d", who, n);
    *px = *tiles = 0;
    for (int i = 0; i < n; i++) {
        if (heights[i] <= 0 || widths[i] <= 0)
            return fail(RF_E_BADARG, "%s: bad size of image %d: h=%d w=%d", who, i, heights[i],
                        widths[i]);
        *px += (size_t)heights[i] * widths[i];
        *tiles += (size_t)ceil_div(heights[i], 64) * ceil_div(widths[i], 64);
        if (*px > ((size_t)1 << 60))
            return fail(RF_E_BADARG, "%s: the images hold too many pixels", who);
    }
    if (int bad = jbf_check_format(who, joint_cn, src_cn, border))
        return bad;
    if (flags & ~kJbfPublicFlags)
        return fail(RF_E_BADARG, "%s: unknown flag bits 0x%x", who, flags);
    const int radius = jbf_radius(d, jbf_sigma(sigma_space));
    if (radius > kJbfMaxRadius)
        return fail(RF_E_UNSUPPORTED, "%s: radius %d too large", who, radius);
    // every tile kernel runs 1024 threads per tile, and the tile records of all classes share one launch
    // rule: refused here, before any table, copy or launch
    if (!launch_fits(*tiles, 1024))
        return fail(RF_E_UNSUPPORTED, "%s: too many tiles for one launch", who);
    return RF_OK;
}

size_t ragged_bytes(size_t tiles) { return (tiles * sizeof(JbfTileRec) + 255) & ~(size_t)255; }

}  // namespace
}  // namespace rf

extern "C" size_t rf_jbf_ragged_workspace_bytes(int n, const int *heights, const int *widths,
                                                int joint_cn, int src_cn, int d, double sigma_space,
                                                int flags)
{
    using namespace rf;
    size_t px, tiles;
    if (ragged_check("rf_jbf_ragged_workspace_bytes", n, heights, widths, joint_cn, src_cn, d,
                     sigma_space, RF_BORDER_DEFAULT, flags, &px, &tiles) != RF_OK)
        return 0;
    return ragged_bytes(tiles);
}

extern "C" int rf_debug_jbf_ragged_plan(int n, const int *heights, const int *widths, int joint_cn,
                                        int src_cn, int d, double sigma_color, double sigma_space,
                                        int flags, int *out, int cap)
{
    using namespace rf;
    size_t px, tiles;
    if (cap < 0 || (cap > 0 && !out))
        return fail(RF_E_BADARG, "rf_debug_jbf_ragged_plan: bad cap=%d", cap);
    if (int bad = ragged_check("rf_debug_jbf_ragged_plan", n, heights, widths, joint_cn, src_cn, d,
                               sigma_space, RF_BORDER_DEFAULT, flags, &px, &tiles))
        return bad;
    std::vector<float> lut;
    const JbfTables t = jbf_host_tables(jbf_radius(d, jbf_sigma(sigma_space)),
                                        jbf_table_cn(joint_cn, flags), jbf_sigma(sigma_color),
                                        jbf_sigma(sigma_space), lut);
    RaggedPlan plan;
    plan_ragged(t, n, heights, widths, src_cn, flags | jbf_debug_flags(),
                debug_get(kDbgJbfTune) & 0xf, &plan);
    if (!plan.tiled)
        return -1;
    int launches = 0;
    for (int c = 0; c < kRaggedClasses; c++) {
        if (plan.recs[c].empty())
            continue;
        if (launches < cap) {
            out[4 * launches + 0] = kRaggedTh[c];
            out[4 * launches + 1] = 4096 / kRaggedTh[c];
            out[4 * launches + 2] = plan.shape.tlw == 144 ? kRaggedPitch144[c] : plan.shape.tlw;
            out[4 * launches + 3] = (int)std::min<size_t>(plan.recs[c].size(), 0x7fffffff);
        }
        launches++;
    }
    return launches;
}

extern "C" int rf_debug_jbf_ragged_slab_plan(int n, const int *heights, const int *widths,
                                             int joint_cn, int src_cn, int d, double sigma_color,
                                             double sigma_space, int flags, int *out, int cap)
{
    using namespace rf;
    const char *who = "rf_debug_jbf_ragged_slab_plan";
    size_t px, tiles;
    if (cap < 0 || (cap > 0 && !out))
        return fail(RF_E_BADARG, "%s: bad cap=%d", who, cap);
    if (int bad = ragged_check(who, n, heights, widths, joint_cn, src_cn, d, sigma_space,
                               RF_BORDER_DEFAULT, flags, &px, &tiles))
        return bad;
    std::vector<float> lut;
    const JbfTables t = jbf_host_tables(jbf_radius(d, jbf_sigma(sigma_space)),
                                        jbf_table_cn(joint_cn, flags), jbf_sigma(sigma_color),
                                        jbf_sigma(sigma_space), lut);
    RaggedPlan plan;
    plan_ragged(t, n, heights, widths, src_cn, flags | jbf_debug_flags(),
                debug_get(kDbgJbfTune) & 0xf, &plan);
    if (!plan.slab)
        return -1;
    if (cap > 0) {
        const SlabShape &s = plan.slab_shape;
        const int record[7] = {s.tlw, s.grep, s.crows_g, s.slab_g, s.crows_c, s.slab_c,
                               (int)std::min<size_t>(plan.recs[0].size(), 0x7fffffff)};
        std::copy(record, record + 7, out);
    }
    return 1;
}

extern "C" int rf_debug_jbf_two_wg_plan(int n, int h, int w, int joint_cn, int src_cn, int d,
                                        double sigma_color, double sigma_space, int flags, int *out)
{
    using namespace rf;
    const char *who = "rf_debug_jbf_two_wg_plan";
    size_t px, tiles;
    if (n < 1 || !out)
        return fail(RF_E_BADARG, "%s: bad n=%d or NULL out", who, n);
    if (int bad = ragged_check(who, 1, &h, &w, joint_cn, src_cn, d, sigma_space, RF_BORDER_DEFAULT, flags,
                               &px, &tiles))
        return bad;
    std::vector<float> lut;
    const JbfTables t = jbf_host_tables(jbf_radius(d, jbf_sigma(sigma_space)),
                                        jbf_table_cn(joint_cn, flags), jbf_sigma(sigma_color),
                                        jbf_sigma(sigma_space), lut);
    flags |= jbf_debug_flags();
    const int nz = t.lut_len < 256 * t.joint_cn ? t.lut_len - 1 : t.lut_len;
    out[0] = out[1] = out[2] = out[3] = 0;
    int slab_rows = 0;
    Tile64Shape shape;
    if (t.r4 > kJbfMaxTiledR4 || !two_wg_choose(t, nz, src_cn, flags, &slab_rows) ||
        !tile64_choose(t, nz, src_cn, flags, &shape))
        return 0;
    const Tile64Areas a = tile64_areas(t, nz, shape.grep, shape.crep, src_cn, flags, h, w);
    const long long blocks = (long long)ceil_div(a.cols_main, 64) * ceil_div(a.rows_main, 64) * n;
    if (a.rows_main <= 0 || a.cols_main <= 0 || !launch_fits(blocks, 1024))
        return 0;
    out[0] = 1;
    out[1] = 64 + slab_rows - 1;
    out[2] = (int)blocks;
    out[3] = src_cn == 3 || joint_cn == 3 ? (int)tile_flag_bytes((size_t)blocks) : 0;
    return 1;
}

extern "C" int rf_jbf_ragged_u8(const uint8_t *joint, const uint8_t *src, uint8_t *dst, int n,
                                const int *heights, const int *widths, int joint_cn, int src_cn,
                                int d, double sigma_color, double sigma_space, int border, int flags,
                                void *workspace, size_t workspace_bytes, void *stream_)
{
    using namespace rf;
    const char *who = "rf_jbf_ragged_u8";
    if (n == 0)  // an empty list is valid whatever the (possibly NULL) pointers are
        return RF_OK;
    if (!joint || !src || !dst)
        return fail(RF_E_BADARG, "%s: NULL image pointer", who);
    size_t px, tiles;
    if (int bad = ragged_check(who, n, heights, widths, joint_cn, src_cn, d, sigma_space, border,
                               flags, &px, &tiles))
        return bad;
    if (ranges_overlap(dst, px * src_cn, joint, px * joint_cn) ||
        ranges_overlap(dst, px * src_cn, src, px * src_cn))
        return fail(RF_E_BADARG, "%s: dst must not overlap an input", who);
    if (!workspace || workspace_bytes < ragged_bytes(tiles) || ((uintptr_t)workspace & 15))
        return fail(RF_E_BADARG, "%s: workspace of %zu bytes, %zu needed (16-byte aligned)", who,
                    workspace ? workspace_bytes : (size_t)0, ragged_bytes(tiles));
    hipStream_t stream = (hipStream_t)stream_;
    if (stream_is_capturing(stream))
        return fail(RF_E_UNSUPPORTED, "%s: synchronises its stream and cannot be captured into a "
                                      "graph", who);
    const int user_flags = flags;
    flags |= jbf_debug_flags();
    const double sc = jbf_sigma(sigma_color), ss = jbf_sigma(sigma_space);
    const int radius = jbf_radius(d, ss);
    const int jcn_kernel = jbf_kernel_cn(joint_cn, flags);
    const int table_cn = jbf_table_cn(joint_cn, flags);
    const int tune = debug_get(kDbgJbfTune) & 0xf;
    RaggedPlan plan;
    JbfTables t;
    TablesHold hold{t};
    // (nothing tiled holds r4 > 468: such a call needs no tables here, rf_jbf_u8 fetches its own)
    if (!(flags & RF_JBF_FORCE_GENERIC) && tune == 0 && ((radius + 3) & ~3) <= kJbfMaxTiledR4) {
        int rc = get_tables(radius, table_cn, sc, ss, stream, &t);
        if (rc != RF_OK)
            return rc;
        bool oob_ok = false;
        rc = lds_oob_reads_zero(t.device, &oob_ok);
        if (rc != RF_OK)
            return rc;
        if (oob_ok)
            plan_ragged(t, n, heights, widths, src_cn, flags, tune, &plan);
    }
    if (!plan.tiled && !plan.slab) {
        // every other route (generic kernel, failed LDS probe, a tuning override):
        // the uniform entry once per image - the same bytes with n launches
        size_t first = 0;
        for (int i = 0; i < n; i++) {
            const int rc = rf_jbf_u8(joint + first * joint_cn, src + first * src_cn,
                                     dst + first * src_cn, 1, heights[i], widths[i], joint_cn, src_cn,
                                     d, sigma_color, sigma_space, border, user_flags, stream_);
            if (rc != RF_OK)
                return rc;
            first += (size_t)heights[i] * widths[i];
        }
        return RF_OK;
    }
    // ---- the tile records of all classes, one after another, copied with one call ---------
    std::vector<JbfTileRec> image;
    const JbfTileRec *d_recs[kRaggedClasses];
    for (int c = 0; c < kRaggedClasses; c++) {
        d_recs[c] = static_cast<const JbfTileRec *>(workspace) + image.size();
        image.insert(image.end(), plan.recs[c].begin(), plan.recs[c].end());
    }
    if (image.size() > tiles)
        return fail(RF_E_HIP, "%s: tile count mismatch (internal)", who);
    // the host image must outlive the copy: the copy is waited for before the launches (this is
    // the call's one synchronisation of `stream`)
    RF_HIP_CHECK(hipMemcpyAsync(workspace, image.data(), image.size() * sizeof(JbfTileRec),
                                hipMemcpyHostToDevice, stream));
    RF_HIP_CHECK(hipStreamSynchronize(stream));
    const int nz = t.lut_len < 256 * table_cn ? t.lut_len - 1 : t.lut_len;
    int rc = RF_OK;
    if (plan.slab) {
        const SlabShape &shp = plan.slab_shape;
#define RF_SLAB(R4_, TLW_)                                                                        \
    if (shp.tlw == TLW_)                                                                          \
        rc = shp.grep == 16                                                                       \
                 ? launch_slab_ragged<16, TLW_>(t, nz, shp, joint, src, dst, d_recs[0],           \
                                                plan.recs[0].size(), jcn_kernel, src_cn, border,  \
                                                flags, stream)                                    \
                 : launch_slab_ragged<8, TLW_>(t, nz, shp, joint, src, dst, d_recs[0],            \
                                               plan.recs[0].size(), jcn_kernel, src_cn, border,   \
                                               flags, stream);
        RF_SLAB_PITCHES(RF_SLAB)
#undef RF_SLAB
        if (rc != RF_OK)
            return rc;
        RF_HIP_CHECK(hipGetLastError());
        return RF_OK;
    }
#define RF_T64(G_, C_, W_)                                                                        \
    if (plan.shape.grep == G_ && plan.shape.crep == C_ && plan.shape.tlw == W_)                   \
        rc = src_cn == 3 ? launch_ragged<3, G_, C_, W_>(t, nz, plan, joint, src, dst, d_recs,      \
                                                        jcn_kernel, border, flags, stream)        \
                         : launch_ragged<1, G_, C_, W_>(t, nz, plan, joint, src, dst, d_recs,      \
                                                        jcn_kernel, border, flags, stream);
    RF_T64_SHAPES(RF_T64)
#undef RF_T64
    if (rc != RF_OK)
        return rc;
    RF_HIP_CHECK(hipGetLastError());
    return RF_OK;
}
#undef RF_SLAB_PITCHES
