// rf_png.hip -- PNG encode on the device, for gfx950: packed 8-bit images of different sizes to one
// finished zlib stream per image (the body of a PNG's IDAT), in three launches per call.
//
// The raw stream of an image is the one image_utils._png_encode filters on the host: per row the
// filter byte 2 (Up) and w * c_out bytes of `pixel - pixel above` mod 256 (zeros above the first
// row), channels in RGB order.  It is cut into chunks of kChunk bytes (the last one shorter) that
// are deflated independently, one workgroup per chunk:
//
//   * tokens: a literal, or a length of 3..258 at distance 1 (a run of the previous byte - what
//     zlib's Z_RLE finds).  After the first byte of a run of equal bytes the repeats are cut into
//     groups of 258; a group of 3 or more is one match, a shorter one literals.  No match reaches
//     behind the chunk's first byte.
//   * one dynamic-Huffman block (BFINAL = 0): HLIT up to the highest used symbol, one distance
//     code of one bit (HDIST = 0), HCLEN = 19 with length 4 for the code-length symbols 0..15 and
//     0 for 16..18 - a complete code, so every literal/length code length is written as four bits.
//     The literal/length code is the Huffman code of the chunk's own histogram (end-of-block counts
//     once), limited to 15 bits by moving codes on the per-length counts until the Kraft sum is
//     exactly 1 again (zlib refuses an incomplete literal/length set).
//   * then an empty stored block (000, pad to a byte, 00 00 FF FF): every chunk ends on a byte
//     and the chunks concatenate by bytes.
//   * a chunk whose dynamic form would be longer than 5 + len bytes is one stored block instead.
//
// The zlib stream of an image is 78 01, its chunks, 03 00 (an empty final fixed block) and the
// Adler-32 of the raw stream, combined from per-chunk partial sums.  Every byte is a function of
// the input alone: the LDS atomics used (integer add, or, max) commute, and nothing depends on the
// order workgroups run in.
#include <vector>

#include "reflectance_filtering_debug.h"
#include "rf_common.hpp"

namespace rf {
namespace {

constexpr int kChunk = 32768;             // raw bytes per chunk (<= 65535: one stored block holds it)
constexpr int kThreads = 512;             // of the deflate kernel
constexpr int kSeg = kChunk / kThreads;   // consecutive raw bytes one thread tokenises (64)
constexpr int kSegDw = kSeg / 4;
constexpr int kRawPitch = kThreads + 1;   // dword d of thread t's segment sits at d * kRawPitch + t
constexpr int kSlotStride = (kChunk + 9 + 15) & ~15;   // bytes between the slots of an image's chunks
constexpr int kSyms = 286;
constexpr int kEob = 256;
constexpr int kMaxBits = 15;
constexpr unsigned kAdlerMod = 65521;
constexpr unsigned long long kMaxChunks = (1ull << 23) - 1;   // 512 threads each, below 2^32 threads
static_assert(kSeg * kThreads == kChunk && kSeg % 4 == 0, "whole dwords per thread");
static_assert(kChunk <= 65535, "a stored block holds at most 65535 bytes");

// One image of a call: where its pixels start in the packed input, its raw stream, the first of its
// chunks in the one-dimensional grid and the first byte of its slots in the workspace.
struct PngImage {
    unsigned long long first;   // pixels before the image
    unsigned long long slot0;   // byte offset of its first chunk's slot in the slot area
    unsigned int rawlen;        // h * (1 + w * c_out)
    unsigned int rowlen;        // 1 + w * c_out
    unsigned int w;
    unsigned int chunk0;
    unsigned int nchunks;
    unsigned int pad;
};
static_assert(sizeof(PngImage) == 40, "the workspace holds 40 bytes per image");

// The image a workgroup works on: the last one with chunk0 <= blockIdx.x (scalar loads only).
__device__ __forceinline__ int image_of_chunk(const PngImage *__restrict__ images, int n)
{
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (images[mid].chunk0 <= blockIdx.x)
            lo = mid;
        else
            hi = mid - 1;
    }
    return lo;
}

// ---- the deflate kernel's pieces ---------------------------------------------------------------

// LDS address (in bytes) of raw byte p of the chunk: segments are interleaved by dwords so that the
// lanes of a wave, each walking its own segment, read consecutive banks.
__device__ __forceinline__ int raw_addr(int p)
{
    return (((p >> 2) & (kSegDw - 1)) * kRawPitch + (p / kSeg)) * 4 + (p & 3);
}

// Inclusive scan over the workgroup's threads in index order (reverse = from the last thread down).
template <bool kReverse, class Op>
__device__ __forceinline__ unsigned block_scan(unsigned v, unsigned *buf, Op op)
{
    const int t = kReverse ? kThreads - 1 - (int)threadIdx.x : (int)threadIdx.x;
    __syncthreads();   // buf may still be read by an earlier scan
    buf[t] = v;
    __syncthreads();
    for (int d = 1; d < kThreads; d <<= 1) {
        const bool on = t >= d;
        const unsigned o = on ? buf[t - d] : 0u;
        __syncthreads();
        if (on) {
            v = op(v, o);
            buf[t] = v;
        }
        __syncthreads();
    }
    return v;
}

// OR `nbits` bits of v into the block image at bit position pos (deflate packs from bit 0 up).
__device__ __forceinline__ void put_at(unsigned *out, unsigned pos, unsigned v, int nbits)
{
    const unsigned long long x = (unsigned long long)v << (pos & 31);
    atomicOr(&out[pos >> 5], (unsigned)x);
    if ((pos & 31) + nbits > 32)
        atomicOr(&out[(pos >> 5) + 1], (unsigned)(x >> 32));
}

// The tokens whose first byte lies in [a, b) of a chunk of len bytes, in order: emit(symbol, number
// of extra bits, their value, 1 for a match).  s_in is the first byte of the run that holds byte a
// (used where byte a continues a run), e_out the end of the run that holds byte b - 1.
template <class Emit>
__device__ __forceinline__ void walk_tokens(const uint8_t *raw, int a, int b, int s_in, int e_out,
                                            Emit emit)
{
    int i = a;
    int s = (a == 0 || raw[raw_addr(a)] != raw[raw_addr(a - 1)]) ? a : s_in;
    while (i < b) {
        // the run [s, e) that holds byte i
        const unsigned v = raw[raw_addr(i)];
        int e = i + 1;
        while (e < b && raw[raw_addr(e)] == v)
            e++;
        if (e == b)
            e = e_out;
        const int stop = e < b ? e : b;
        const int repeats = e - s - 1;
        int p = i;
        while (p < stop) {
            if (p == s) {
                emit(v, 0, 0u, 0);
                p++;
                continue;
            }
            const int j = p - s - 1;
            const int g = j / 258, k = j - g * 258;
            const int rest = repeats - g * 258;
            const int glen = rest < 258 ? rest : 258;
            if (glen < 3) {
                emit(v, 0, 0u, 0);
                p++;
            } else {
                if (k == 0) {
                    const int l = glen - 3;
                    if (l < 8) {
                        emit(257u + l, 0, 0u, 1);
                    } else if (glen == 258) {
                        emit(285u, 0, 0u, 1);
                    } else {
                        const int eb = 29 - __clz(l);   // floor(log2(l)) - 2: 1..5
                        emit(261u + 4 * eb + ((l >> eb) & 3), eb, (unsigned)l & ((1u << eb) - 1), 1);
                    }
                }
                p += glen - k;   // the rest of the group is covered by its match
            }
        }
        i = stop;
        s = stop;
    }
}

// Minimum-redundancy code lengths (Moffat and Katajainen's in-place algorithm) of the n >= 2
// frequencies in A, sorted ascending; A[i] becomes the length of the i-th code.  One lane.
__device__ void huffman_lengths(unsigned *A, int n)
{
    A[0] += A[1];
    int root = 0, leaf = 2;
    for (int next = 1; next < n - 1; next++) {
        if (leaf >= n || A[root] < A[leaf]) {
            A[next] = A[root];
            A[root++] = next;
        } else {
            A[next] = A[leaf++];
        }
        if (leaf >= n || (root < next && A[root] < A[leaf])) {
            A[next] += A[root];
            A[root++] = next;
        } else {
            A[next] += A[leaf++];
        }
    }
    A[n - 2] = 0;
    for (int next = n - 3; next >= 0; next--)
        A[next] = A[A[next]] + 1;
    int avbl = 1, used = 0, dpth = 0;
    root = n - 2;
    int next = n - 1;
    while (avbl > 0) {
        while (root >= 0 && (int)A[root] == dpth) {
            used++;
            root--;
        }
        while (avbl > used) {
            A[next--] = dpth;
            avbl--;
        }
        avbl = 2 * used;
        dpth++;
        used = 0;
    }
}

struct DeflateShared {
    unsigned raw[kSegDw * kRawPitch];      // the chunk's raw bytes, segments interleaved
    unsigned out[kChunk / 4 + 4];          // the dynamic block's image (used up to len + 5 bytes)
    unsigned scan[kThreads];
    unsigned hist[288];
    unsigned work[288];                    // sorted frequencies, then code lengths in that order
    unsigned short order[288];             // symbols by ascending (frequency, symbol)
    unsigned short codes[288];             // bit-reversed Huffman codes
    unsigned char lens[288];
    unsigned numc[kMaxBits + 1];           // codes per length
    unsigned base[kMaxBits + 1];           // first code of each length
    unsigned nused, maxsym, adler_a, adler_b, total_bits;
};

// One raw byte of an image: the Up difference of sample `col - 1` of row `row` (col 0: the filter
// byte).  px is the image's first pixel; cn_in / grey_as_rgb select the input form.
__device__ __forceinline__ unsigned raw_byte(const uint8_t *__restrict__ px, unsigned row,
                                             unsigned col, unsigned w, int cn_in, bool grey_as_rgb)
{
    if (col == 0)
        return 2u;
    const unsigned k = col - 1;
    size_t idx;
    unsigned pitch;
    if (cn_in == 3) {
        const unsigned x = k / 3;
        idx = ((size_t)row * w + x) * 3 + (2 - (k - x * 3));   // BGR in memory, RGB in the file
        pitch = w * 3;
    } else {
        idx = (size_t)row * w + (grey_as_rgb ? k / 3 : k);
        pitch = w;
    }
    const unsigned cur = px[idx];
    const unsigned up = row ? px[idx - pitch] : 0u;
    return (cur - up) & 255u;
}

__global__ __launch_bounds__(kThreads) void png_deflate_kernel(
    const uint8_t *__restrict__ pixels, const PngImage *__restrict__ images, int n, int cn_in,
    int grey_as_rgb, uint8_t *__restrict__ slots, unsigned *__restrict__ chunk_bytes,
    unsigned *__restrict__ chunk_adler)
{
    __shared__ DeflateShared sh;
    const int tid = threadIdx.x;
    const int img = image_of_chunk(images, n);
    const PngImage im = images[img];
    const unsigned c = blockIdx.x - im.chunk0;
    const unsigned base = c * (unsigned)kChunk;   // < rawlen < 2^31
    const int len = (int)(im.rawlen - base < (unsigned)kChunk ? im.rawlen - base : (unsigned)kChunk);
    const uint8_t *px = pixels + im.first * (size_t)cn_in;

    for (int i = tid; i < 288; i += kThreads) {
        sh.hist[i] = i == kEob ? 1u : 0u;
        sh.lens[i] = 0;
    }
    for (int i = tid; i < kChunk / 4 + 4; i += kThreads)
        sh.out[i] = 0;
    if (tid == 0) {
        sh.nused = 0;
        sh.maxsym = kEob;
        sh.adler_a = 0;
        sh.adler_b = 0;
    }

    // ---- the raw bytes, four per step, and the Adler partial sums of the chunk ----
    unsigned ad_a = 0, ad_b = 0;   // sum of d, sum of (len - position) * d; below 2^32 (16 steps)
    for (int q = tid; q < kChunk / 4; q += kThreads) {
        const int p = q * 4;
        unsigned word = 0;
        if (p < len) {
            const unsigned o = base + (unsigned)p;
            unsigned row = o / im.rowlen, col = o - row * im.rowlen;
            unsigned sum = 0, wsum = 0;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                if (p + k < len) {
                    const unsigned d = raw_byte(px, row, col, im.w, cn_in, grey_as_rgb != 0);
                    word |= d << (8 * k);
                    sum += d;
                    wsum += d * k;
                    if (++col == im.rowlen) {
                        col = 0;
                        row++;
                    }
                }
            }
            ad_a += sum;
            ad_b += (unsigned)(len - p) * sum - wsum;
        }
        sh.raw[(q & (kSegDw - 1)) * kRawPitch + q / kSegDw] = word;
    }
    __syncthreads();
    atomicAdd(&sh.adler_a, ad_a % kAdlerMod);   // at most 512 * 65520 each
    atomicAdd(&sh.adler_b, ad_b % kAdlerMod);

    // ---- runs of equal bytes across the threads' segments ----
    const uint8_t *raw = reinterpret_cast<const uint8_t *>(sh.raw);
    const int a = tid * kSeg;
    const int b = a + kSeg < len ? a + kSeg : len;   // b <= a: nothing of the chunk is this thread's
    unsigned first_break = 0x7fffffffu, last_break = 0;   // positions + 1 for the max scan, 0 = none
    for (int i = a; i < b; i++) {
        if (i == 0 || raw[raw_addr(i)] != raw[raw_addr(i - 1)]) {
            if (first_break == 0x7fffffffu)
                first_break = (unsigned)i;
            last_break = (unsigned)i + 1;
        }
    }
    if (a >= len)
        first_break = (unsigned)len;   // the chunk's end ends its last run
    // the start of the run that reaches into the segment: the last break of the threads before
    unsigned incl = block_scan<false>(last_break, sh.scan,
                                      [](unsigned x, unsigned y) { return x > y ? x : y; });
    __syncthreads();
    sh.scan[tid] = incl;
    __syncthreads();
    const int s_in = tid > 0 ? (int)sh.scan[tid - 1] - 1 : 0;
    // the end of the run that leaves the segment: the first break of the threads after (0 stands
    // for "none" in the scan, so positions are stored complemented)
    incl = block_scan<true>(0x7fffffffu - first_break, sh.scan,
                            [](unsigned x, unsigned y) { return x > y ? x : y; });
    __syncthreads();
    sh.scan[tid] = incl;
    __syncthreads();
    int e_out = tid + 1 < kThreads ? (int)(0x7fffffffu - sh.scan[tid + 1]) : len;
    if (e_out > len)
        e_out = len;

    // ---- histogram ----
    walk_tokens(raw, a, b, s_in, e_out, [&](unsigned sym, int, unsigned, int) {
        atomicAdd(&sh.hist[sym], 1u);
    });
    __syncthreads();

    // ---- code lengths: rank sort of the used symbols, the tree on one lane, the 15-bit limit ----
    for (int t = tid; t < kSyms; t += kThreads) {
        const unsigned f = sh.hist[t];
        if (f == 0)
            continue;
        int rank = 0;
        for (int u = 0; u < kSyms; u++) {
            const unsigned g = sh.hist[u];
            rank += (g != 0 && (g < f || (g == f && u < t))) ? 1 : 0;
        }
        sh.order[rank] = (unsigned short)t;
        sh.work[rank] = f;
        atomicAdd(&sh.nused, 1u);
        atomicMax(&sh.maxsym, (unsigned)t);
    }
    __syncthreads();
    if (tid == 0) {
        const int nu = (int)sh.nused;   // >= 2: end-of-block and at least one token
        huffman_lengths(sh.work, nu);
        for (int i = 0; i <= kMaxBits; i++)
            sh.numc[i] = 0;
        for (int i = 0; i < nu; i++) {
            const unsigned l = sh.work[i];
            sh.numc[l < kMaxBits ? l : kMaxBits]++;   // deeper codes move up to 15 bits ...
        }
        unsigned total = 0;
        for (int i = kMaxBits; i >= 1; i--)
            total += sh.numc[i] << (kMaxBits - i);
        while (total != (1u << kMaxBits)) {   // ... and the Kraft sum comes back down to exactly 1
            sh.numc[kMaxBits]--;
            for (int i = kMaxBits - 1; i >= 1; i--) {
                if (sh.numc[i]) {
                    sh.numc[i]--;
                    sh.numc[i + 1] += 2;
                    break;
                }
            }
            total--;
        }
        int j = nu;   // the most frequent symbols take the shortest codes
        for (int i = 1; i <= kMaxBits; i++)
            for (unsigned l = sh.numc[i]; l > 0; l--)
                sh.lens[sh.order[--j]] = (unsigned char)i;
        unsigned code = 0;
        sh.base[0] = 0;
        for (int i = 1; i <= kMaxBits; i++) {
            code = (code + sh.numc[i - 1]) << 1;
            sh.base[i] = code;
        }
    }
    __syncthreads();
    for (int t = tid; t < kSyms; t += kThreads) {
        const unsigned l = sh.lens[t];
        if (l == 0)
            continue;
        unsigned idx = 0;
        for (int u = 0; u < t; u++)
            idx += sh.lens[u] == l ? 1u : 0u;
        sh.codes[t] = (unsigned short)(__brev(sh.base[l] + idx) >> (32 - l));
    }
    __syncthreads();

    // ---- bit offsets ----
    const unsigned hlit = sh.maxsym + 1;   // >= 257
    const unsigned hbits = 3 + 5 + 5 + 4 + 19 * 3 + 4 * hlit + 4;
    unsigned mybits = 0;
    walk_tokens(raw, a, b, s_in, e_out, [&](unsigned sym, int eb, unsigned, int match) {
        mybits += sh.lens[sym] + eb + match;
    });
    incl = block_scan<false>(mybits, sh.scan, [](unsigned x, unsigned y) { return x + y; });
    if (tid == kThreads - 1)
        sh.total_bits = hbits + incl + sh.lens[kEob];
    __syncthreads();
    const unsigned end_bits = sh.total_bits;                        // header, tokens, end-of-block
    const unsigned dyn_bytes = ((end_bits + 3 + 7) >> 3) + 4;       // ... and the empty stored block
    const bool stored = dyn_bytes > 5u + (unsigned)len;
    const unsigned nbytes = stored ? 5u + (unsigned)len : dyn_bytes;
    uint8_t *slot = slots + im.slot0 + (size_t)c * kSlotStride;

    if (stored) {
        if (tid == 0) {
            slot[0] = 0;   // BFINAL = 0, BTYPE = 00, padding
            slot[1] = (uint8_t)(len & 255);
            slot[2] = (uint8_t)(len >> 8);
            slot[3] = (uint8_t)(~len & 255);
            slot[4] = (uint8_t)((~len >> 8) & 255);
        }
        for (int p = tid; p < len; p += kThreads)
            slot[5 + p] = raw[raw_addr(p)];
    } else {
        // header: BFINAL = 0, BTYPE = 10 | HLIT | HDIST = 0 | HCLEN = 15 | 19 x 3 bits in the order
        // 16 17 18 0 8 7 ...: 0 0 0 and sixteen 4s | the code lengths, four bits each, as codes of
        // the code-length code (symbol v has the 4-bit code v, packed from its highest bit)
        if (tid == 0) {
            put_at(sh.out, 0, 4u | ((hlit - 257) << 3) | (15u << 13), 17);
            put_at(sh.out, 17 + 9, 0x924924u, 24);        // eight 3-bit fields holding 4
            put_at(sh.out, 17 + 9 + 24, 0x924924u, 24);   // and eight more
            put_at(sh.out, 74 + 4 * hlit, __brev(1u) >> 28, 4);   // the one distance code: length 1
            put_at(sh.out, end_bits - sh.lens[kEob], sh.codes[kEob], sh.lens[kEob]);
            put_at(sh.out, 8 * (dyn_bytes - 2), 0xFFFFu, 16);     // the empty stored block: 00 00 FF FF
        }
        for (unsigned t = tid; t < hlit; t += kThreads)
            put_at(sh.out, 74 + 4 * t, __brev((unsigned)sh.lens[t]) >> 28, 4);
        // tokens: at most 15 + 5 + 1 bits each, gathered in a 64-bit window, one OR per dword
        const unsigned pos = hbits + incl - mybits;
        unsigned wpos = pos >> 5;
        int fill = (int)(pos & 31);
        unsigned long long acc = 0;
        walk_tokens(raw, a, b, s_in, e_out, [&](unsigned sym, int eb, unsigned extra, int match) {
            const int l = sh.lens[sym];
            const unsigned v = sh.codes[sym] | (extra << l);   // the distance code is the bit 0
            acc |= (unsigned long long)v << fill;
            fill += l + eb + match;
            if (fill >= 32) {
                atomicOr(&sh.out[wpos++], (unsigned)acc);
                acc >>= 32;
                fill -= 32;
            }
        });
        if (acc != 0)
            atomicOr(&sh.out[wpos], (unsigned)acc);
        __syncthreads();
        unsigned *slot32 = reinterpret_cast<unsigned *>(slot);   // slots are 16-byte aligned
        for (unsigned i = tid; i < (nbytes + 3) / 4; i += kThreads)
            slot32[i] = sh.out[i];
    }
    if (tid == 0) {
        chunk_bytes[blockIdx.x] = nbytes;
        chunk_adler[2 * (size_t)blockIdx.x] = sh.adler_a % kAdlerMod;
        chunk_adler[2 * (size_t)blockIdx.x + 1] = sh.adler_b % kAdlerMod;
    }
}

// ---- layout: where every chunk and every stream goes, and the Adler-32 of every image ----------

__device__ __forceinline__ unsigned long long wave_scan_incl(unsigned long long v, int lane)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned long long o = __shfl_up(v, d, 64);
        if (lane >= d)
            v += o;
    }
    return v;
}

constexpr int kLayoutThreads = 1024;

// One workgroup.  Each wave takes every 16th image: the exclusive scan of its chunk sizes (from 2:
// the zlib header) into chunk_off, its stream size into image_bytes and its Adler-32 into
// image_adler; then the first wave scans the stream sizes into stream_offsets[n + 1].
__global__ __launch_bounds__(kLayoutThreads) void png_layout_kernel(
    const PngImage *__restrict__ images, int n, const unsigned *__restrict__ chunk_bytes,
    const unsigned *__restrict__ chunk_adler, unsigned *__restrict__ chunk_off,
    unsigned *__restrict__ image_bytes, unsigned *__restrict__ image_adler,
    unsigned long long *__restrict__ stream_offsets)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int i = wave; i < n; i += kLayoutThreads / 64) {
        const PngImage im = images[i];
        unsigned long long run = 2, sa = 0, sb = 0;
        for (unsigned c0 = 0; c0 < im.nchunks; c0 += 64) {
            const unsigned c = c0 + lane;
            const bool on = c < im.nchunks;
            const unsigned long long sz = on ? chunk_bytes[im.chunk0 + c] : 0;
            const unsigned long long incl = wave_scan_incl(sz, lane);
            if (on) {
                chunk_off[im.chunk0 + c] = (unsigned)(run + incl - sz);
                // with B = sum of (chunk length - position) * d over a chunk, the bytes behind the
                // chunk add their count times the chunk's sum of d
                const unsigned long long end =
                    (unsigned long long)(c + 1) * kChunk < im.rawlen ? (unsigned long long)(c + 1) * kChunk
                                                                     : im.rawlen;
                const unsigned long long a = chunk_adler[2 * (size_t)(im.chunk0 + c)];
                const unsigned long long b = chunk_adler[2 * (size_t)(im.chunk0 + c) + 1];
                sa += a;
                sb += (b + a * ((im.rawlen - end) % kAdlerMod)) % kAdlerMod;
            }
            run += __shfl(incl, 63, 64);
        }
        sa = __shfl(wave_scan_incl(sa % kAdlerMod, lane), 63, 64);
        sb = __shfl(wave_scan_incl(sb % kAdlerMod, lane), 63, 64);
        if (lane == 0) {
            const unsigned s1 = (unsigned)((1 + sa) % kAdlerMod);            // the sums start at 1, 0
            const unsigned s2 = (unsigned)((sb + im.rawlen % kAdlerMod) % kAdlerMod);
            image_adler[i] = (s2 << 16) | s1;
            image_bytes[i] = (unsigned)(run + 6);   // 03 00 and the Adler-32; below 2^31 by the bound
        }
    }
    __threadfence_block();
    __syncthreads();
    if (wave == 0) {
        unsigned long long run = 0;
        for (int i0 = 0; i0 < n; i0 += 64) {
            const int i = i0 + lane;
            const unsigned long long sz = i < n ? image_bytes[i] : 0;
            const unsigned long long incl = wave_scan_incl(sz, lane);
            if (i < n)
                stream_offsets[i] = run + incl - sz;
            run += __shfl(incl, 63, 64);
        }
        if (lane == 0)
            stream_offsets[n] = run;
    }
}

// ---- gather: slots into contiguous streams ------------------------------------------------------

constexpr int kGatherThreads = 256;

__global__ __launch_bounds__(kGatherThreads) void png_gather_kernel(
    const PngImage *__restrict__ images, int n, const uint8_t *__restrict__ slots,
    const unsigned *__restrict__ chunk_bytes, const unsigned *__restrict__ chunk_off,
    const unsigned *__restrict__ image_adler, const unsigned long long *__restrict__ stream_offsets,
    uint8_t *__restrict__ streams)
{
    const int img = image_of_chunk(images, n);
    const PngImage &im = images[img];
    const unsigned c = blockIdx.x - im.chunk0;
    const unsigned sz = chunk_bytes[blockIdx.x];
    const uint8_t *src = slots + im.slot0 + (size_t)c * kSlotStride;
    uint8_t *image_stream = streams + stream_offsets[img];
    uint8_t *dst = image_stream + chunk_off[blockIdx.x];
    // bytes up to the first aligned dword of dst, whole dwords funnelled out of two aligned source
    // dwords (the slot is 16-byte aligned and 4 bytes longer than any chunk), then the last bytes
    const unsigned head = min((unsigned)(-(uintptr_t)dst & 3), sz);
    const unsigned ndw = (sz - head) / 4;
    const unsigned tail0 = head + 4 * ndw;
    if (threadIdx.x < head)
        dst[threadIdx.x] = src[threadIdx.x];
    const unsigned *src32 = reinterpret_cast<const unsigned *>(src);
    unsigned *dst32 = reinterpret_cast<unsigned *>(dst + head);
    const unsigned shift = 8 * head;   // head is 0..3: the source runs `head` bytes ahead
    for (unsigned j = threadIdx.x; j < ndw; j += kGatherThreads) {
        const unsigned lo = src32[j];
        dst32[j] = shift ? (lo >> shift) | (src32[j + 1] << (32 - shift)) : lo;
    }
    if (threadIdx.x < sz - tail0)
        dst[tail0 + threadIdx.x] = src[tail0 + threadIdx.x];
    if (threadIdx.x == 0) {
        if (c == 0) {
            image_stream[0] = 0x78;   // deflate, 32 KiB window; FLEVEL 0, check bits
            image_stream[1] = 0x01;
        }
        if (c == im.nchunks - 1) {
            const unsigned ad = image_adler[img];
            uint8_t *t = dst + sz;
            t[0] = 0x03;   // BFINAL = 1, BTYPE = 01, end-of-block (seven zero bits)
            t[1] = 0x00;
            t[2] = (uint8_t)(ad >> 24);
            t[3] = (uint8_t)(ad >> 16);
            t[4] = (uint8_t)(ad >> 8);
            t[5] = (uint8_t)ad;
        }
    }
}

// ---- the plan of a call (host) -------------------------------------------------------------------

inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

struct PngPlan {
    std::vector<PngImage> images;
    unsigned long long chunks;   // of all images
    unsigned long long pixels;
    unsigned long long bound;    // stream bytes of all images at most
    unsigned long long slots;    // bytes of the slot area
};

// The workspace: [image table][chunk bytes][chunk offsets][chunk Adler pairs][image bytes]
// [image Adler][slots], each part rounded up to 256 bytes.
struct PngWorkspace {
    size_t chunk_bytes, chunk_off, chunk_adler, image_bytes, image_adler, slots, total;
};

PngWorkspace workspace_layout(const PngPlan &plan)
{
    PngWorkspace ws;
    const size_t n = plan.images.size();
    size_t at = align256(sizeof(PngImage) * n);
    ws.chunk_bytes = at;
    at += align256(4 * (size_t)plan.chunks);
    ws.chunk_off = at;
    at += align256(4 * (size_t)plan.chunks);
    ws.chunk_adler = at;
    at += align256(8 * (size_t)plan.chunks);
    ws.image_bytes = at;
    at += align256(4 * n);
    ws.image_adler = at;
    at += align256(4 * n);
    ws.slots = at;
    ws.total = at + align256((size_t)plan.slots);
    return ws;
}

// The argument rules of the sizes, channels and flags, and the chunks of every image.  The bound of
// an image's stream: 78 01, per chunk its bytes and at most 9 more, 03 00, the Adler-32.
int plan_png(const char *who, int n, const int *heights, const int *widths, int cn_in, int flags,
             PngPlan *plan)
{
    if (n < 0)
        return fail(RF_E_BADARG, "%s: bad size n=%d", who, n);
    if (n > 0 && (!heights || !widths))
        return fail(RF_E_BADARG, "%s: NULL pointer", who);
    if (cn_in != 1 && cn_in != 3)
        return fail(RF_E_UNSUPPORTED, "%s: cn_in=%d (1 or 3 channels)", who, cn_in);
    if (flags & ~RF_PNG_GREY_AS_RGB)
        return fail(RF_E_BADARG, "%s: unknown flag bits 0x%x", who, flags & ~RF_PNG_GREY_AS_RGB);
    if ((flags & RF_PNG_GREY_AS_RGB) && cn_in != 1)
        return fail(RF_E_BADARG, "%s: the flag RF_PNG_GREY_AS_RGB needs cn_in = 1", who);
    const unsigned long long c_out = (cn_in == 3 || (flags & RF_PNG_GREY_AS_RGB)) ? 3 : 1;
    plan->images.resize((size_t)n);
    plan->chunks = plan->pixels = plan->bound = plan->slots = 0;
    for (int i = 0; i < n; i++) {
        if (heights[i] <= 0 || widths[i] <= 0)
            return fail(RF_E_BADARG, "%s: bad size of image %d: h=%d w=%d", who, i, heights[i],
                        widths[i]);
        const unsigned long long rowlen = 1 + (unsigned long long)widths[i] * c_out;
        const unsigned long long rawlen = rowlen * (unsigned long long)heights[i];
        const unsigned long long nch = (rawlen + kChunk - 1) / kChunk;
        const unsigned long long bound = 2 + rawlen + 9 * nch + 2 + 4;
        if (bound >= (1ull << 31))
            return fail(RF_E_UNSUPPORTED, "%s: the stream of image %d (%dx%d) may reach 2^31 bytes: "
                                          "more than one IDAT chunk holds", who, i, widths[i],
                        heights[i]);
        if (plan->chunks + nch > kMaxChunks)
            return fail(RF_E_UNSUPPORTED, "%s: more chunks than one grid takes (%llu)", who,
                        kMaxChunks);
        PngImage &im = plan->images[i];
        im.first = plan->pixels;
        im.slot0 = plan->slots;
        im.rawlen = (unsigned)rawlen;
        im.rowlen = (unsigned)rowlen;
        im.w = (unsigned)widths[i];
        im.chunk0 = (unsigned)plan->chunks;
        im.nchunks = (unsigned)nch;
        im.pad = 0;
        plan->pixels += (unsigned long long)heights[i] * widths[i];
        plan->chunks += nch;
        plan->bound += bound;
        plan->slots += (nch - 1) * kSlotStride + ((rawlen - (nch - 1) * kChunk + 9 + 15) & ~15ull);
    }
    return RF_OK;
}

}  // namespace
}  // namespace rf

extern "C" size_t rf_png_stream_bound(int n, const int *heights, const int *widths, int cn_in,
                                      int flags)
{
    rf::PngPlan plan;
    if (n <= 0 || rf::plan_png("rf_png_stream_bound", n, heights, widths, cn_in, flags, &plan) != RF_OK)
        return 0;
    return (size_t)plan.bound;
}

extern "C" size_t rf_png_workspace_bytes(int n, const int *heights, const int *widths, int cn_in,
                                         int flags)
{
    rf::PngPlan plan;
    if (n <= 0 ||
        rf::plan_png("rf_png_workspace_bytes", n, heights, widths, cn_in, flags, &plan) != RF_OK)
        return 0;
    return rf::workspace_layout(plan).total;
}

extern "C" int rf_debug_png_plan(int n, const int *heights, const int *widths, int cn_in, int flags,
                                 int *out, int cap)
{
    using namespace rf;
    if (cap < 0 || (cap > 0 && !out))
        return fail(RF_E_BADARG, "rf_debug_png_plan: bad cap %d", cap);
    PngPlan plan;
    const int rc = plan_png("rf_debug_png_plan", n, heights, widths, cn_in, flags, &plan);
    if (rc != RF_OK)
        return rc;
    if (cap > 0)
        out[0] = kChunk;
    if (cap > 1)
        out[1] = (int)plan.chunks;
    for (int i = 0; i < n && i + 2 < cap; i++)
        out[i + 2] = (int)plan.images[i].nchunks;
    return n;
}

extern "C" int rf_png_deflate_ragged_u8(const uint8_t *images, int n, const int *heights,
                                        const int *widths, int cn_in, int flags, uint8_t *streams,
                                        size_t stream_capacity, unsigned long long *stream_offsets,
                                        void *workspace, size_t workspace_bytes, void *stream_)
{
    using namespace rf;
    const char *who = "rf_png_deflate_ragged_u8";
    if (n == 0)
        return RF_OK;
    if (!images || !heights || !widths || !streams || !stream_offsets || !workspace)
        return fail(RF_E_BADARG, "%s: NULL pointer", who);
    PngPlan plan;
    const int rc = plan_png(who, n, heights, widths, cn_in, flags, &plan);
    if (rc != RF_OK)
        return rc;
    if (stream_capacity < plan.bound)
        return fail(RF_E_BADARG, "%s: stream capacity %zu B < the bound %llu B", who, stream_capacity,
                    plan.bound);
    const PngWorkspace ws = workspace_layout(plan);
    if (workspace_bytes < ws.total)
        return fail(RF_E_WORKSPACE, "%s: workspace %zu B < %zu B", who, workspace_bytes, ws.total);
    if ((uintptr_t)workspace % 16 != 0)
        return fail(RF_E_BADARG, "%s: the workspace must be 16-byte aligned", who);
    if ((uintptr_t)stream_offsets % 8 != 0)
        return fail(RF_E_BADARG, "%s: stream_offsets must be 8-byte aligned", who);
    if (ranges_overlap(streams, stream_capacity, images, (size_t)plan.pixels * cn_in))
        return fail(RF_E_BADARG, "%s: streams overlap images", who);
    hipStream_t stream = (hipStream_t)stream_;
    if (stream_is_capturing(stream))
        return fail(RF_E_UNSUPPORTED, "%s: synchronises its stream and cannot be captured into a "
                                      "graph", who);
    // the host table must outlive the copy: the copy is waited for before the launches (this is
    // the call's one synchronisation of `stream`)
    RF_HIP_CHECK(hipMemcpyAsync(workspace, plan.images.data(), sizeof(PngImage) * (size_t)n,
                                hipMemcpyHostToDevice, stream));
    RF_HIP_CHECK(hipStreamSynchronize(stream));
    char *wsb = static_cast<char *>(workspace);
    const PngImage *table = reinterpret_cast<const PngImage *>(wsb);
    unsigned *chunk_bytes = reinterpret_cast<unsigned *>(wsb + ws.chunk_bytes);
    unsigned *chunk_off = reinterpret_cast<unsigned *>(wsb + ws.chunk_off);
    unsigned *chunk_adler = reinterpret_cast<unsigned *>(wsb + ws.chunk_adler);
    unsigned *image_bytes = reinterpret_cast<unsigned *>(wsb + ws.image_bytes);
    unsigned *image_adler = reinterpret_cast<unsigned *>(wsb + ws.image_adler);
    uint8_t *slots = reinterpret_cast<uint8_t *>(wsb + ws.slots);
    const dim3 grid((unsigned int)plan.chunks);
    hipLaunchKernelGGL(png_deflate_kernel, grid, dim3(kThreads), 0, stream, images, table, n, cn_in,
                       (flags & RF_PNG_GREY_AS_RGB) ? 1 : 0, slots, chunk_bytes, chunk_adler);
    hipLaunchKernelGGL(png_layout_kernel, dim3(1), dim3(kLayoutThreads), 0, stream, table, n,
                       chunk_bytes, chunk_adler, chunk_off, image_bytes, image_adler, stream_offsets);
    hipLaunchKernelGGL(png_gather_kernel, grid, dim3(kGatherThreads), 0, stream, table, n, slots,
                       chunk_bytes, chunk_off, image_adler, stream_offsets, streams);
    RF_HIP_CHECK(hipGetLastError());
    return RF_OK;
}
