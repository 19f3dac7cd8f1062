// rf_jbf_greymap.hip -- the grey map of rf_jbf_u8's two-workgroups-per-CU route (rf_jbf.hip): the
// route's one byte per 64x64 tile (bit 0 = the src is NOT grey somewhere in the tile's region, bit 1 =
// the joint IS grey everywhere in it) from ONE pass over the images.
//
// A tile's region is its staged rectangle seen through the border rule: rows tile_y0 - radius ..
// tile_y0 + 63 + radius and columns tile_x0 - r4 .. tile_x0 - r4 + 143, each through
// border_interpolate.  Regions overlap - a scan per tile (kJbfVoteOnly in rf_jbf.hip, kept under
// "jbf_vote_scan") reads every texel 4.6 times at radius 33 - but a region is a rectangle of the image
// (border_span), so a pixel says at once which tiles it speaks for: those whose column span holds its
// x, times those whose row span holds its y.  A workgroup reads a block of 256 x 64 pixels of the
// 3-channel buffers (a wave one row of 768 B per load instruction), every lane ORs the column sets of
// its coloured pixels into one word per tile row, the workgroup ORs its lanes' words in LDS and then
// changes the bytes of the tiles it has something to say to: bit 0 set where a src pixel is coloured,
// bit 1 cleared where a joint pixel is.  The bytes start as 2 (jbf_grey_map_clear_kernel, the launch in
// front), so an all-grey batch performs no atomic at all.
#include "rf_jbf_common.hpp"

namespace rf {
namespace {

// The rows (columns) [*lo, *hi] that border_interpolate(p, len, border) takes for p = a .. b, where [a, b]
// holds an index inside [0, len) (a tile's first row or column).  Inside the image the span is itself; rows
// replicated, or reflected at 0, fall on rows the span holds anyway; rows reflected at the far edge reach
// back to 2 len - 1 - b (- 1 for REFLECT_101), which a tile with few rows inside the image does not hold
// itself; past either edge of the image the reflection has swept all of it.  CONSTANT adds zeros: grey.
// (Not for WRAP, whose span is two pieces: such calls keep the scan.)
__host__ __device__ inline void border_span(int a, int b, int len, int border, int *lo, int *hi)
{
    int l = a > 0 ? a : 0, u = b < len - 1 ? b : len - 1;
    if (border == RF_BORDER_REFLECT || border == RF_BORDER_REFLECT_101) {
        const int delta = border == RF_BORDER_REFLECT_101;
        if (a < 0) {
            const int top = -a - 1 + delta;
            u = top > u ? (top < len - 1 ? top : len - 1) : u;
        }
        if (b >= len) {
            const int back = 2 * len - 1 - b - delta;
            l = back < l ? (back > 0 ? back : 0) : l;
        }
    }
    *lo = l;
    *hi = u;
}

// the tiles a 256 x 64 block of pixels (block column gx, block row gy) looks at: tile columns 4 gx - 2 ..
// 4 gx + 7 and tile rows gy - 1 .. gy + 2.  jbf_grey_map_serves checks on the host that no region reaches
// a block that does not look at its tile.
constexpr int kMapCols = 10, kMapRows = 4, kMapColFirst = -2, kMapRowFirst = -1;
constexpr int kMapBatch = 4;  // rows a wave has in flight (per buffer one 12-byte load per lane and row)

// the tile columns (bits of cm[u], the set of pixel u of the quad) that get to know of a coloured pixel
// among the four BGR pixels in the twelve bytes d
__device__ inline uint32_t coloured_columns(const uint32_t (&d)[3], const uint32_t (&cm)[4])
{
    // byte k of e = byte k ^ byte k + 1 of the twelve: a pixel is grey iff both its byte pairs are equal
    const uint32_t e0 = d[0] ^ ((d[0] >> 8) | (d[1] << 24));
    const uint32_t e1 = d[1] ^ ((d[1] >> 8) | (d[2] << 24));
    const uint32_t e2 = d[2] ^ (d[2] >> 8);
    return ((e0 & 0x0000ffffu) ? cm[0] : 0u) | (((e0 & 0xff000000u) | (e1 & 0x000000ffu)) ? cm[1] : 0u) |
           ((e1 & 0xffff0000u) ? cm[2] : 0u) | ((e2 & 0x00ffff00u) ? cm[3] : 0u);
}

// twelve bytes from any address
__device__ inline void load12(const uint8_t *p, uint32_t (&d)[3])
{
    __builtin_memcpy(&d[0], p, 4);
    __builtin_memcpy(&d[1], p + 4, 4);
    __builtin_memcpy(&d[2], p + 8, 4);
}

// the last npx < 4 pixels of a row, byte by byte; the missing ones zero (grey)
__device__ inline void load_row_end(const uint8_t *p, int npx, uint32_t (&d)[3])
{
    d[0] = d[1] = d[2] = 0u;
    for (int k = 0; k < 3 * npx; k++)
        d[k >> 2] |= (uint32_t)p[k] << (8 * (k & 3));
}

__global__ __launch_bounds__(256) void jbf_grey_map_clear_kernel(uint32_t *__restrict__ words, int nwords)
{
    const int i = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (i < nwords)
        words[i] = 0x02020202u;  // every tile: src grey, joint grey
}

// SRC / JOINT: the buffer has three channels (a single-channel buffer is grey and is not read)
template <bool SRC, bool JOINT>
__global__ __launch_bounds__(256) void jbf_grey_map_kernel(
    const uint8_t *__restrict__ joint, const uint8_t *__restrict__ src, int h, int w, int radius, int border,
    int tiles_x, int tiles_y, int blocks_x, int blocks_y, uint32_t *__restrict__ tile_words)
{
    __shared__ uint32_t acc[2 * kMapRows];  // per tile row: columns with a coloured src pixel, then joint
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid < 2 * kMapRows)
        acc[tid] = 0u;
    const int gx = (int)(blockIdx.x % (unsigned)blocks_x);
    const int gy = (int)((blockIdx.x / (unsigned)blocks_x) % (unsigned)blocks_y);
    const int img_idx = (int)(blockIdx.x / ((unsigned)blocks_x * (unsigned)blocks_y));
    const int r4 = (radius + 3) & ~3;
    const int x = 256 * gx + 4 * lane;
    // the lane's four pixels: which of the block's tile columns hold each in their span
    uint32_t cm[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int c = 0; c < kMapCols; c++) {
        const int tx = 4 * gx + kMapColFirst + c;
        if (tx < 0 || tx >= tiles_x)
            continue;
        int lo, hi;
        border_span(64 * tx - r4, 64 * tx - r4 + 143, w, border, &lo, &hi);
#pragma unroll
        for (int u = 0; u < 4; u++)
            cm[u] |= (x + u >= lo && x + u <= hi) ? 1u << c : 0u;
    }
    // the row spans of the block's tile rows (empty: no such tile row)
    int ylo[kMapRows], yhi[kMapRows];
#pragma unroll
    for (int r = 0; r < kMapRows; r++) {
        const int ty = gy + kMapRowFirst + r;
        ylo[r] = 1, yhi[r] = 0;
        if (ty >= 0 && ty < tiles_y)
            border_span(64 * ty - radius, 64 * ty + 63 + radius, h, border, &ylo[r], &yhi[r]);
    }
    __syncthreads();
    uint32_t as[kMapRows] = {0u, 0u, 0u, 0u}, aj[kMapRows] = {0u, 0u, 0u, 0u};
    const size_t img = (size_t)img_idx * h * w;
    // (a lane outside every span - one beyond the image's right edge, too - loads nothing; a span lies inside
    //  the image, so a set bit says x < w)
    const bool active = (cm[0] | cm[1] | cm[2] | cm[3]) != 0u;
    if (active && w - x >= 4) {
        for (int i0 = 0; i0 < 16; i0 += kMapBatch) {
            const int y0 = 64 * gy + wave + 4 * i0;  // (the wave's row: the same in every lane)
            if (y0 >= h)
                break;
            // rows below the image: the last row again, which no span test below lets through
            uint32_t ds[kMapBatch][3], dj[kMapBatch][3];
#pragma unroll
            for (int k = 0; k < kMapBatch; k++) {
                const int yc = min(y0 + 4 * k, h - 1);
                const size_t at = (img + (size_t)yc * w + x) * 3;
                if (SRC)
                    load12(src + at, ds[k]);
                if (JOINT)
                    load12(joint + at, dj[k]);
            }
#pragma unroll
            for (int k = 0; k < kMapBatch; k++) {
                const int y = y0 + 4 * k;
                const uint32_t cs = SRC ? coloured_columns(ds[k], cm) : 0u;
                const uint32_t cj = JOINT ? coloured_columns(dj[k], cm) : 0u;
#pragma unroll
                for (int r = 0; r < kMapRows; r++)
                    if (y >= ylo[r] && y <= yhi[r])
                        as[r] |= cs, aj[r] |= cj;
            }
        }
    } else if (active) {
        // the one lane per row that holds the last w % 4 pixels
        for (int i = 0; i < 16; i++) {
            const int y = 64 * gy + wave + 4 * i;
            if (y >= h)
                break;
            const size_t at = (img + (size_t)y * w + x) * 3;
            uint32_t cs = 0u, cj = 0u, d[3];
            if (SRC) {
                load_row_end(src + at, w - x, d);
                cs = coloured_columns(d, cm);
            }
            if (JOINT) {
                load_row_end(joint + at, w - x, d);
                cj = coloured_columns(d, cm);
            }
#pragma unroll
            for (int r = 0; r < kMapRows; r++)
                if (y >= ylo[r] && y <= yhi[r])
                    as[r] |= cs, aj[r] |= cj;
        }
    }
#pragma unroll
    for (int r = 0; r < kMapRows; r++) {
        if (as[r])
            atomicOr(&acc[r], as[r]);
        if (aj[r])
            atomicOr(&acc[kMapRows + r], aj[r]);
    }
    __syncthreads();
    if (tid < kMapRows * kMapCols) {
        const int r = tid / kMapCols, c = tid - r * kMapCols;
        const int tx = 4 * gx + kMapColFirst + c, ty = gy + kMapRowFirst + r;
        if (tx >= 0 && tx < tiles_x && ty >= 0 && ty < tiles_y) {
            const int tile = (img_idx * tiles_y + ty) * tiles_x + tx;
            const int shift = 8 * (tile & 3);
            if ((acc[r] >> c) & 1u)
                atomicOr(&tile_words[tile >> 2], 1u << shift);
            if ((acc[kMapRows + r] >> c) & 1u)
                atomicAnd(&tile_words[tile >> 2], ~(2u << shift));
        }
    }
}

}  // namespace

// Does the map kernel reach every tile of the tiles_x x tiles_y tiles of an h x w image?  Every block that
// a tile's region touches must look at that tile.  (The scan serves the calls it does not hold for.)
bool jbf_grey_map_serves(int h, int w, int radius, int border, int tiles_x, int tiles_y)
{
    if (border == RF_BORDER_WRAP)
        return false;
    const int r4 = (radius + 3) & ~3;
    for (int tx = 0; tx < tiles_x; tx++) {
        int lo, hi;
        border_span(64 * tx - r4, 64 * tx - r4 + 143, w, border, &lo, &hi);
        for (int gx = lo / 256; gx <= hi / 256; gx++)
            if (tx < 4 * gx + kMapColFirst || tx >= 4 * gx + kMapColFirst + kMapCols)
                return false;
    }
    for (int ty = 0; ty < tiles_y; ty++) {
        int lo, hi;
        border_span(64 * ty - radius, 64 * ty + 63 + radius, h, border, &lo, &hi);
        for (int gy = lo / 64; gy <= hi / 64; gy++)
            if (ty < gy + kMapRowFirst || ty >= gy + kMapRowFirst + kMapRows)
                return false;
    }
    return true;
}

// The tile bytes of the tiles_x x tiles_y tiles of every image's main area: the bytes' words set to "grey",
// then one pass over all h x w pixels of the 3-channel buffers (jcn, scn: 3, or anything else for a
// single-channel buffer).  tile_flags: the route's buffer, a power of two of at least 4 KiB.
int jbf_launch_grey_map(const uint8_t *joint, const uint8_t *src, int n, int h, int w, int jcn, int scn,
                        int radius, int border, hipStream_t stream, int tiles_x, int tiles_y,
                        uint8_t *tile_flags)
{
    const int blocks_x = ceil_div(w, 256), blocks_y = ceil_div(h, 64);
    const long long blocks = (long long)blocks_x * blocks_y * n;
    if (!launch_fits(blocks, 256))
        return fail(RF_E_UNSUPPORTED, "rf_jbf_u8: batch too large for one launch");
    const int nwords = (int)(((long long)tiles_x * tiles_y * n + 3) / 4);  // (whole words: the buffer's size rule)
    uint32_t *words = reinterpret_cast<uint32_t *>(tile_flags);
    hipLaunchKernelGGL(jbf_grey_map_clear_kernel, dim3((unsigned)ceil_div(nwords, 256)), dim3(256), 0, stream,
                       words, nwords);
    if (scn != 3 && jcn != 3)
        return RF_OK;
    auto kern = scn == 3 && jcn == 3 ? jbf_grey_map_kernel<true, true>
                : scn == 3           ? jbf_grey_map_kernel<true, false>
                                     : jbf_grey_map_kernel<false, true>;
    hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(256), 0, stream, joint, src, h, w, radius, border,
                       tiles_x, tiles_y, blocks_x, blocks_y, words);
    return RF_OK;
}

}  // namespace rf
