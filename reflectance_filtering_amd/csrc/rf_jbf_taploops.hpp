// rf_jbf_taploops.hpp -- the tap loops of the tiled joint bilateral kernels (rf_jbf.hip, which
// describes the pipeline under "Tiled kernels").  Device only: every loop takes LDS byte addresses
// and accumulates one lane's kPix horizontally adjacent outputs.
//   jbf_tap_loop            the software-pipelined loop, compiler-scheduled VALU (any texel form)
//   jbf_tap_loop_grey4      hand-interleaved form for grey tiles, gathers one column step ahead
//   jbf_tap_loop_grey4_la2  the same two column steps ahead: the default grey loop (SLAB: slab kernel)
//   jbf_tap_loop_rgb6       hand-interleaved colour loop on 6-byte texels
// Every macro defined here is #undef-ed again below.
#pragma once
#include <type_traits>

#include "rf_common.hpp"

namespace rf {
namespace {

constexpr int kPix = 4;        // outputs per lane (horizontal)

typedef uint32_t uint2v __attribute__((ext_vector_type(2)));
typedef float float4v __attribute__((ext_vector_type(4)));

// The LDS reads of the tap loop are issued through asm so that their order and their waits are
// exactly the pipeline described above (left to itself the compiler sinks each read next to its
// use and waits for lgkmcnt(0) after every gather).  The wait statement names everything it
// releases -- and the accumulators -- as in/out operands: that keeps consumers below the wait
// and the accumulation of the current column above it, i.e. underneath the reads in flight.
#define RF_LDS_READ_B64(dst, addr, off) \
    asm volatile("ds_read_b64 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "n"(off))
#define RF_LDS_READ_B128(dst, addr, off) \
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "n"(off))
#define RF_LDS_READ_B32(dst, addr) asm volatile("ds_read_b32 %0, %1" : "=v"(dst) : "v"(addr))
#define RF_LDS_READ_B32_OFF(dst, addr, off) \
    asm volatile("ds_read_b32 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "n"(off))
#define RF_LDS_READ_U16_OFF(dst, addr, off) \
    asm volatile("ds_read_u16 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "n"(off))

// Accumulates all taps of one lane's 4 outputs.  NCH = channels accumulated (3, or 1 when the
// src is single-channel or every src texel of the tile is grey: identical bits, a third of the
// multiply-adds).  TB = bytes per LDS texel: 8 = {BGRx joint, BGRx src}; 4 = {B,G,R joint, grey
// src} (NCH = 1 only).  CLAMP = clamp the LUT index with v_min (otherwise the caller guarantees
// that every reachable index is either inside the staged table or beyond the end of the
// workgroup's LDS allocation, where ds_read returns 0).  sum/wsum must be zero on entry.
template <int NCH, int LUTREP, bool CLAMP, int TLW, int TB>
__device__ __forceinline__ void jbf_tap_loop(uint32_t lut_lane_addr, uint32_t sw_addr0,
                                             uint32_t tile_lane_addr, uint32_t plane_b_lane_addr,
                                             const uint32_t (&jc)[kPix], uint32_t amax, int ty,
                                             int radius, int r4, int sw_len,
                                             const int *__restrict__ hwtab, float (&sum)[kPix][NCH],
                                             float (&wsum)[kPix])
{
    static_assert((TB == 8) || (TB == 4 && NCH == 1) || (TB == 6 && NCH == 3),
                  "4-byte texels carry one src channel, 6-byte ones three");
    constexpr int TA = TB == 6 ? 4 : TB;  // bytes per texel in the main plane
    constexpr int Q4 = TLW / 4;
    using texel_t = typename std::conditional<TB == 8, uint2v, uint32_t>::type;
    auto joint_of = [](const texel_t &t) -> uint32_t {
        if constexpr (TB == 8)
            return t.x;
        else
            return t & 0x00ffffffu;
    };
    // all four addresses first, then the four reads back to back: LDS instructions issued in
    // a cluster disturb the VALU stream less than reads interleaved with their address math
    // (+2.8 % on the hand-scheduled grey loop, in-process A/B)
    auto issue_gathers = [&](uint32_t jtex, float *g) {
        uint32_t a[kPix];
#pragma unroll
        for (int p = 0; p < kPix; p++) {
            uint32_t alpha = __builtin_amdgcn_sad_u8(jtex, jc[p], 0u);
            if (CLAMP)
                alpha = min(alpha, amax);
            a[p] = alpha * (LUTREP * 4u) + lut_lane_addr;
        }
        asm volatile("" : "+v"(a[0]), "+v"(a[1]), "+v"(a[2]), "+v"(a[3]));
#pragma unroll
        for (int p = 0; p < kPix; p++)
            RF_LDS_READ_B32(g[p], a[p]);
    };
    // TB == 6: second plane of 2-byte texels {G src, R src}; U = ring slot
#define RF_READ_TEXEL(U, off_texels)                                   \
    if constexpr (TB == 8) {                                           \
        RF_LDS_READ_B64(tq[U], ta, (off_texels) * 8);                  \
    } else {                                                           \
        RF_LDS_READ_B32_OFF(tq[U], ta, (off_texels) * 4);              \
        if constexpr (TB == 6)                                         \
            RF_LDS_READ_U16_OFF(tqb[U], tb, (off_texels) * 2);         \
    }

    for (int i = -radius; i <= radius; i++) {
        const int hw = hwtab[i + radius];
        const int hw4 = (hw + 3) & ~3;
        const int ai = i < 0 ? -i : i;
        // column c = 4*gq + u - hw4 (gq = 0 .. hw4/2): tile column X = c + r4 + 4*tx, i.e. texel
        // address = ta + (u*Q4 + gq)*TB with ta the per-lane address of (row, group 0, u = 0)
        const uint32_t texel0 = (uint32_t)((ty + i + radius) * TLW + ((r4 - hw4) >> 2));
        uint32_t ta = tile_lane_addr + texel0 * TA;
        uint32_t tb = plane_b_lane_addr + texel0 * 2;
        // weight of tap (i, j) = swc[j] = swc[-j]; group gq needs swc[hw4 - 4*gq - 4 .. +3]
        uint32_t wa_addr = sw_addr0 + (uint32_t)((ai * sw_len + (r4 + 8) + hw4 - 4) * 4);
        const int ngroups = (hw4 >> 1) + 1;

        // Register rings with compile-time indices only: column 4*gq+u lives in tq[u], its
        // gathers in gg[u & 1].  Every read issued in a step is released by the wait at the END
        // of that step, so nothing is in flight across the loop back-edge (a value in flight
        // there would be copied by the compiler's phi moves before it has landed).
        texel_t tq[4];
        uint32_t tqb[4] = {0u, 0u, 0u, 0u};  // second plane (TB == 6 only)
        float4v wna, wnb;
        float gg[2][kPix];
        RF_READ_TEXEL(0, 0)
        RF_READ_TEXEL(1, Q4)
        RF_LDS_READ_B128(wna, wa_addr, 0);
        RF_LDS_READ_B128(wnb, wa_addr, 16);
        asm volatile("s_waitcnt lgkmcnt(0)"
                     : "+v"(tq[0]), "+v"(tq[1]), "+v"(tqb[0]), "+v"(tqb[1]), "+v"(wna), "+v"(wnb));
        issue_gathers(joint_of(tq[0]), gg[0]);
        asm volatile("s_waitcnt lgkmcnt(0)"
                     : "+v"(gg[0][0]), "+v"(gg[0][1]), "+v"(gg[0][2]), "+v"(gg[0][3]));

#define RF_ACCUM(U)                                                                  \
    {                                                                                \
        float s[NCH];                                                                \
        if constexpr (TB == 8) {                                                     \
            const uint32_t sv = tq[(U)].y;                                           \
            s[0] = (float)(sv & 0xff);                                               \
            if constexpr (NCH == 3) {                                                \
                s[1] = (float)((sv >> 8) & 0xff);                                    \
                s[2] = (float)((sv >> 16) & 0xff);                                   \
            }                                                                        \
        } else {                                                                     \
            s[0] = (float)(tq[(U)] >> 24);                                           \
            if constexpr (TB == 6) {                                                 \
                s[1] = (float)(tqb[(U)] & 0xff);                                     \
                s[2] = (float)((tqb[(U)] >> 8) & 0xff);                              \
            }                                                                        \
        }                                                                            \
        _Pragma("unroll") for (int p = 0; p < kPix; p++)                             \
        {                                                                            \
            const float wgt = __fmul_rn(wv[4 + p - (U)], gg[(U) & 1][p]);            \
            _Pragma("unroll") for (int ch = 0; ch < NCH; ch++) sum[p][ch] =          \
                __fadd_rn(sum[p][ch], __fmul_rn(wgt, s[ch]));                        \
            wsum[p] = __fadd_rn(wsum[p], wgt);                                       \
        }                                                                            \
    }
#define RF_TEXEL_OFF(U) ((((U) + 2) & 3) * Q4 + (((U) + 2) >> 2))
        // Pins the accumulators at this point of the instruction stream (no instruction).
#define RF_PIN_ACC()                                                                            \
    if constexpr (NCH == 3) {                                                                   \
        asm volatile(""                                                                         \
                     : "+v"(sum[0][0]), "+v"(sum[1][0]), "+v"(sum[2][0]), "+v"(sum[3][0]),      \
                       "+v"(sum[0][1]), "+v"(sum[1][1]), "+v"(sum[2][1]), "+v"(sum[3][1]),      \
                       "+v"(sum[0][NCH - 1]), "+v"(sum[1][NCH - 1]), "+v"(sum[2][NCH - 1]),     \
                       "+v"(sum[3][NCH - 1]), "+v"(wsum[0]), "+v"(wsum[1]), "+v"(wsum[2]),      \
                       "+v"(wsum[3]));                                                          \
    } else {                                                                                    \
        asm volatile(""                                                                         \
                     : "+v"(sum[0][0]), "+v"(sum[1][0]), "+v"(sum[2][0]), "+v"(sum[3][0]),      \
                       "+v"(wsum[0]), "+v"(wsum[1]), "+v"(wsum[2]), "+v"(wsum[3]));             \
    }
        // one column: issue texel(+2) and gathers(+1), accumulate column +0 underneath them,
        // then release what was issued
#define RF_STEP(U)                                                                            \
    RF_READ_TEXEL(((U) + 2) & 3, RF_TEXEL_OFF(U))                                             \
    issue_gathers(joint_of(tq[((U) + 1) & 3]), gg[((U) + 1) & 1]);                            \
    __builtin_amdgcn_sched_barrier(0);                                                        \
    RF_ACCUM(U)                                                                               \
    __builtin_amdgcn_sched_barrier(0);                                                        \
    RF_PIN_ACC()                                                                              \
    __builtin_amdgcn_sched_barrier(0);                                                        \
    asm volatile("s_waitcnt lgkmcnt(0)"                                                       \
                 : "+v"(tq[((U) + 2) & 3]), "+v"(tqb[((U) + 2) & 3]),                         \
                   "+v"(gg[((U) + 1) & 1][0]), "+v"(gg[((U) + 1) & 1][1]),                    \
                   "+v"(gg[((U) + 1) & 1][2]), "+v"(gg[((U) + 1) & 1][3]));                   \
    __builtin_amdgcn_sched_barrier(0);

        for (int gq = 0; gq < ngroups; gq++) {
            float wv[8];
            wv[0] = wna.x; wv[1] = wna.y; wv[2] = wna.z; wv[3] = wna.w;
            wv[4] = wnb.x; wv[5] = wnb.y; wv[6] = wnb.z; wv[7] = wnb.w;
            RF_STEP(0)
            RF_STEP(1)
            RF_STEP(2)
            // u = 3 also fetches the next group's weight window
            RF_READ_TEXEL(1, RF_TEXEL_OFF(3))
            issue_gathers(joint_of(tq[0]), gg[0]);
            wa_addr -= 16;
            RF_LDS_READ_B128(wna, wa_addr, 0);
            RF_LDS_READ_B128(wnb, wa_addr, 16);
            __builtin_amdgcn_sched_barrier(0);
            RF_ACCUM(3)
            __builtin_amdgcn_sched_barrier(0);
            RF_PIN_ACC()
            __builtin_amdgcn_sched_barrier(0);
            asm volatile("s_waitcnt lgkmcnt(0)"
                         : "+v"(tq[1]), "+v"(tqb[1]), "+v"(wna), "+v"(wnb), "+v"(gg[0][0]),
                           "+v"(gg[0][1]), "+v"(gg[0][2]), "+v"(gg[0][3]));
            __builtin_amdgcn_sched_barrier(0);
            ta += TA;
            tb += 2;
        }
#undef RF_STEP
#undef RF_PIN_ACC
#undef RF_ACCUM
#undef RF_TEXEL_OFF
    }
#undef RF_READ_TEXEL
}

// Hand-scheduled tap loop for grey tiles (4-byte texels, one accumulated channel), same
// arithmetic and the same pipeline as jbf_tap_loop<1, LUTREP, false, TLW, 4>.
//
// Why asm: a gfx950 SIMD retires two wave-instructions per 4 cycles only if at most one of them
// is a "full-pipe" opcode (v_sad_u8, v_lshl_add_u32, v_cvt_*, anything with an SGPR/constant
// operand ...; 4 cycles each back to back) and the other a "simple" one (v_mul_f32 / v_add_f32 /
// v_and_b32 on VGPRs; 2 cycles each) -- tools/microbench/valu_rates2.hip.  Per column this loop
// needs 9 full-pipe and 17 simple instructions; hipcc emits them as an 8-instruction full-pipe
// burst followed by the simple ones, the blocks below interleave them one for one.
// J1: the joint has one channel and its texel field holds the value pre-multiplied by the LUT's
// byte stride (3x that for RF_JBF_GREY_AS_BGR), so v_sad_u32(texel, centre, lane address) IS the
// gather address: no v_lshl_add_u32, 22 instead of 26 VALU instructions per column step.
template <int LUTREP, int TLW, bool J1 = false>
__device__ __forceinline__ void jbf_tap_loop_grey4(uint32_t lut_lane_addr, uint32_t sw_addr0,
                                                   uint32_t tile_lane_addr,
                                                   const uint32_t (&jc)[kPix], int ty, int radius,
                                                   int r4, int sw_len,
                                                   const int *__restrict__ hwtab,
                                                   float (&sum)[kPix][1], float (&wsum)[kPix])
{
    constexpr int Q4 = TLW / 4;
    constexpr int SHIFT = LUTREP == 32 ? 7 : LUTREP == 16 ? 6 : LUTREP == 8 ? 5 : 4;
    static_assert(LUTREP == 32 || LUTREP == 16 || LUTREP == 8 || LUTREP == 4, "LUT replicas");
    uint32_t mask = 0x00ffffffu;
    asm volatile("" : "+v"(mask));  // keep the mask in a VGPR (a literal operand is full-pipe)

    // Row geometry: the lane's first texel address and the address of the first weight window.
    auto row_addr = [&](int i, uint32_t &ta_out, uint32_t &wa_out, int &ngroups_out) {
        const int hw = hwtab[i + radius];
        const int hw4 = (hw + 3) & ~3;
        const int ai = i < 0 ? -i : i;
        ta_out = tile_lane_addr + (uint32_t)(((ty + i + radius) * TLW + ((r4 - hw4) >> 2)) * 4);
        wa_out = sw_addr0 + (uint32_t)((ai * sw_len + (r4 + 8) + hw4 - 4) * 4);
        ngroups_out = (hw4 >> 1) + 1;
    };

    // look-ahead texels of columns 0..3 of a group as two register pairs: columns (0, 1) and
    // (2, 3) are each fetched by one ds_read2_b32 (their tile addresses differ by Q4 texels)
    uint2v tp[2];
    float4v wna, wnb;
    float gg[2][kPix];
    uint32_t ta, wa_addr;
    int ngroups;
    row_addr(-radius, ta, wa_addr, ngroups);
    // prologue of the first tap row: texels of columns 0 and 1, weight window of group 0,
    // gathers of column 0.  Every later row gets these from the last group of the row before.
    asm volatile("ds_read2_b32 %0, %1 offset1:%2" : "=&v"(tp[0]) : "v"(ta), "n"(Q4));
    asm volatile("ds_read_b128 %0, %2\n\t"
                 "ds_read_b128 %1, %2 offset:16"
                 : "=&v"(wna), "=&v"(wnb)
                 : "v"(wa_addr));
    asm volatile("s_waitcnt lgkmcnt(2)" : "+v"(tp[0]));
    {
        const uint32_t tj = tp[0].x & mask;
#pragma unroll
        for (int p = 0; p < kPix; p++) {
            const uint32_t a =
                J1 ? (tj > jc[p] ? tj - jc[p] : jc[p] - tj) + lut_lane_addr
                   : __builtin_amdgcn_sad_u8(tj, jc[p], 0u) * (LUTREP * 4u) + lut_lane_addr;
            asm volatile("ds_read_b32 %0, %1" : "=v"(gg[0][p]) : "v"(a));
        }
    }
    asm volatile("s_waitcnt lgkmcnt(0)"
                 : "+v"(tp[0]), "+v"(wna), "+v"(wnb), "+v"(gg[0][0]), "+v"(gg[0][1]),
                   "+v"(gg[0][2]), "+v"(gg[0][3]));

    // even steps fetch the texels of two columns (this step's look-ahead and the next step's);
    // the pair is an output of the even steps only
#define RF_TQ(U) tp[((U) & 3) >> 1][(U) & 1]
#define RF_G4_TNOUT(U) RF_G4_TNOUT_##U
#define RF_G4_TNOUT_0 [tn] "=&v"(tp[1]),
#define RF_G4_TNOUT_2 [tn] "=&v"(tp[0]),
#define RF_G4_TNOUT_1
#define RF_G4_TNOUT_3
#define RF_G4_READ(U) RF_G4_READ_##U
#define RF_G4_READ_0 "ds_read2_b32 %[tn], %[ta] offset0:%[o0] offset1:%[o1]\n\t"
#define RF_G4_READ_2 "ds_read2_b32 %[tn], %[ta] offset0:%[o0] offset1:%[o1]\n\t"
#define RF_G4_READ_1 ""
#define RF_G4_READ_3 ""
#define RF_TEXEL_OFF4(U) (((((U) + 2) & 3) * Q4 + (((U) + 2) >> 2)) * 4)
    // Column step U of a group: texel of column +2 (from address TA + OFF), SAD + gathers of
    // column +1, accumulation of column +0.  GA = gathers being consumed, GB = gathers being
    // issued (their registers first hold alpha, then the LDS address, then the LUT value).
#define RF_G4_PART1(U, GA, GB, TA, OFF, OFF1)                                                          \
    float w0_, w1_, w2_, w3_, s_;                                                                \
    uint32_t tj_;                                                                                \
    asm volatile(RF_G4_READ(U)                                                                   \
                 "v_and_b32 %[tj], %[mask], %[t1]\n\t"                                           \
                 "v_sad_u8 %[a0], %[tj], %[jc0], 0\n\t"                                          \
                 "v_mul_f32 %[w0], %[wv0], %[g0]\n\t"                                            \
                 "v_sad_u8 %[a1], %[tj], %[jc1], 0\n\t"                                          \
                 "v_mul_f32 %[w1], %[wv1], %[g1]\n\t"                                            \
                 "v_sad_u8 %[a2], %[tj], %[jc2], 0\n\t"                                          \
                 "v_mul_f32 %[w2], %[wv2], %[g2]\n\t"                                            \
                 "v_sad_u8 %[a3], %[tj], %[jc3], 0\n\t"                                          \
                 "v_mul_f32 %[w3], %[wv3], %[g3]\n\t"                                            \
                 "v_cvt_f32_ubyte3 %[s], %[t0]"                                                  \
                 : RF_G4_TNOUT(U)[tj] "=&v"(tj_), [a0] "=&v"(GB[0]),                             \
                   [a1] "=&v"(GB[1]), [a2] "=&v"(GB[2]), [a3] "=&v"(GB[3]), [w0] "=&v"(w0_),     \
                   [w1] "=&v"(w1_), [w2] "=&v"(w2_), [w3] "=&v"(w3_), [s] "=&v"(s_)              \
                 : [ta] "v"(TA), [o0] "n"((OFF) / 4), [o1] "n"((OFF1) / 4), [mask] "v"(mask),    \
                   [t1] "v"(RF_TQ((U) + 1)), [t0] "v"(RF_TQ(U)), [jc0] "v"(jc[0]),               \
                   [jc1] "v"(jc[1]), [jc2] "v"(jc[2]), [jc3] "v"(jc[3]), [wv0] "v"(wv[4 - (U)]), \
                   [wv1] "v"(wv[5 - (U)]), [wv2] "v"(wv[6 - (U)]), [wv3] "v"(wv[7 - (U)]),       \
                   [g0] "v"(GA[0]), [g1] "v"(GA[1]), [g2] "v"(GA[2]), [g3] "v"(GA[3]));          \
    asm volatile("v_lshl_add_u32 %[a0], %[a0], %[sh], %[la]\n\t"                                 \
                 "v_add_f32 %[ws0], %[ws0], %[w0]\n\t"                                           \
                 "v_lshl_add_u32 %[a1], %[a1], %[sh], %[la]\n\t"                                 \
                 "v_add_f32 %[ws1], %[ws1], %[w1]\n\t"                                           \
                 "v_lshl_add_u32 %[a2], %[a2], %[sh], %[la]\n\t"                                 \
                 "v_add_f32 %[ws2], %[ws2], %[w2]\n\t"                                           \
                 "v_lshl_add_u32 %[a3], %[a3], %[sh], %[la]\n\t"                                 \
                 "v_add_f32 %[ws3], %[ws3], %[w3]\n\t"                                           \
                 "ds_read_b32 %[a0], %[a0]\n\t"                                                  \
                 "ds_read_b32 %[a1], %[a1]\n\t"                                                  \
                 "ds_read_b32 %[a2], %[a2]\n\t"                                                  \
                 "ds_read_b32 %[a3], %[a3]"                                                      \
                 : [a0] "+v"(GB[0]), [a1] "+v"(GB[1]), [a2] "+v"(GB[2]), [a3] "+v"(GB[3]),       \
                   [ws0] "+v"(wsum[0]), [ws1] "+v"(wsum[1]), [ws2] "+v"(wsum[2]),                \
                   [ws3] "+v"(wsum[3])                                                           \
                 : [sh] "n"(SHIFT), [la] "v"(lut_lane_addr), [w0] "v"(w0_), [w1] "v"(w1_),       \
                   [w2] "v"(w2_), [w3] "v"(w3_));
    // the same step for a single-channel joint (J1): the SAD of the pre-scaled values plus the
    // lane's LUT address is the gather address
#define RF_G4_PART1_J1(U, GA, GB, TA, OFF, OFF1)                                                       \
    float w0_, w1_, w2_, w3_, s_;                                                                \
    uint32_t tj_;                                                                                \
    asm volatile(RF_G4_READ(U)                                                                   \
                 "v_and_b32 %[tj], %[mask], %[t1]\n\t"                                           \
                 "v_sad_u32 %[a0], %[tj], %[jc0], %[la]\n\t"                                     \
                 "v_mul_f32 %[w0], %[wv0], %[g0]\n\t"                                            \
                 "v_sad_u32 %[a1], %[tj], %[jc1], %[la]\n\t"                                     \
                 "v_mul_f32 %[w1], %[wv1], %[g1]\n\t"                                            \
                 "v_sad_u32 %[a2], %[tj], %[jc2], %[la]\n\t"                                     \
                 "v_mul_f32 %[w2], %[wv2], %[g2]\n\t"                                            \
                 "v_sad_u32 %[a3], %[tj], %[jc3], %[la]\n\t"                                     \
                 "v_mul_f32 %[w3], %[wv3], %[g3]\n\t"                                            \
                 "v_cvt_f32_ubyte3 %[s], %[t0]"                                                  \
                 : RF_G4_TNOUT(U)[tj] "=&v"(tj_), [a0] "=&v"(GB[0]),                             \
                   [a1] "=&v"(GB[1]), [a2] "=&v"(GB[2]), [a3] "=&v"(GB[3]), [w0] "=&v"(w0_),     \
                   [w1] "=&v"(w1_), [w2] "=&v"(w2_), [w3] "=&v"(w3_), [s] "=&v"(s_)              \
                 : [ta] "v"(TA), [o0] "n"((OFF) / 4), [o1] "n"((OFF1) / 4), [mask] "v"(mask),    \
                   [la] "v"(lut_lane_addr),                                                      \
                   [t1] "v"(RF_TQ((U) + 1)), [t0] "v"(RF_TQ(U)), [jc0] "v"(jc[0]),               \
                   [jc1] "v"(jc[1]), [jc2] "v"(jc[2]), [jc3] "v"(jc[3]), [wv0] "v"(wv[4 - (U)]), \
                   [wv1] "v"(wv[5 - (U)]), [wv2] "v"(wv[6 - (U)]), [wv3] "v"(wv[7 - (U)]),       \
                   [g0] "v"(GA[0]), [g1] "v"(GA[1]), [g2] "v"(GA[2]), [g3] "v"(GA[3]));          \
    asm volatile("v_add_f32 %[ws0], %[ws0], %[w0]\n\t"                                           \
                 "v_add_f32 %[ws1], %[ws1], %[w1]\n\t"                                           \
                 "v_add_f32 %[ws2], %[ws2], %[w2]\n\t"                                           \
                 "v_add_f32 %[ws3], %[ws3], %[w3]\n\t"                                           \
                 "ds_read_b32 %[a0], %[a0]\n\t"                                                  \
                 "ds_read_b32 %[a1], %[a1]\n\t"                                                  \
                 "ds_read_b32 %[a2], %[a2]\n\t"                                                  \
                 "ds_read_b32 %[a3], %[a3]"                                                      \
                 : [a0] "+v"(GB[0]), [a1] "+v"(GB[1]), [a2] "+v"(GB[2]), [a3] "+v"(GB[3]),       \
                   [ws0] "+v"(wsum[0]), [ws1] "+v"(wsum[1]), [ws2] "+v"(wsum[2]),                \
                   [ws3] "+v"(wsum[3])                                                           \
                 : [w0] "v"(w0_), [w1] "v"(w1_), [w2] "v"(w2_), [w3] "v"(w3_));
#define RF_G4_PART2(TN, GB, EXTRA_OPERANDS)                                                      \
    asm volatile("v_mul_f32 %[w0], %[w0], %[s]\n\t"                                              \
                 "v_mul_f32 %[w1], %[w1], %[s]\n\t"                                              \
                 "v_mul_f32 %[w2], %[w2], %[s]\n\t"                                              \
                 "v_mul_f32 %[w3], %[w3], %[s]\n\t"                                              \
                 "v_add_f32 %[s0], %[s0], %[w0]\n\t"                                             \
                 "v_add_f32 %[s1], %[s1], %[w1]\n\t"                                             \
                 "v_add_f32 %[s2], %[s2], %[w2]\n\t"                                             \
                 "v_add_f32 %[s3], %[s3], %[w3]\n\t"                                             \
                 "s_waitcnt lgkmcnt(0)"                                                          \
                 : [w0] "+v"(w0_), [w1] "+v"(w1_), [w2] "+v"(w2_), [w3] "+v"(w3_),               \
                   [s0] "+v"(sum[0][0]), [s1] "+v"(sum[1][0]), [s2] "+v"(sum[2][0]),             \
                   [s3] "+v"(sum[3][0]), "+v"(TN), "+v"(GB[0]), "+v"(GB[1]), "+v"(GB[2]),        \
                   "+v"(GB[3]) EXTRA_OPERANDS                                                    \
                 : [s] "v"(s_));
#define RF_COMMA_W , "+v"(wna), "+v"(wnb)
#define RF_LOAD_WINDOW(ADDR)                                                                     \
    asm volatile("ds_read_b128 %0, %2\n\t"                                                       \
                 "ds_read_b128 %1, %2 offset:16"                                                 \
                 : "=&v"(wna), "=&v"(wnb)                                                        \
                 : "v"(ADDR));

#define RF_ROW_LOOP(P1)                                                            \
    for (int i = -radius; i <= radius; i++) {                                                       \
        uint32_t ta_next, wa_next;                                                                  \
        int ngroups_next;                                                                           \
        row_addr(i < radius ? i + 1 : i, ta_next, wa_next, ngroups_next);                           \
        for (int gq = 0; gq < ngroups - 1; gq++) {                                                  \
            float wv[8];                                                                            \
            wv[0] = wna.x; wv[1] = wna.y; wv[2] = wna.z; wv[3] = wna.w;                             \
            wv[4] = wnb.x; wv[5] = wnb.y; wv[6] = wnb.z; wv[7] = wnb.w;                             \
            {                                                                                       \
                P1(0, gg[0], gg[1], ta, RF_TEXEL_OFF4(0), RF_TEXEL_OFF4(1))                         \
                RF_G4_PART2(tp[1], gg[1], )                                                         \
            }                                                                                       \
            {                                                                                       \
                P1(1, gg[1], gg[0], ta, 0, 0)                                                       \
                RF_G4_PART2(tp[1], gg[0], )                                                         \
            }                                                                                       \
            {                                                                                       \
                P1(2, gg[0], gg[1], ta, RF_TEXEL_OFF4(2), RF_TEXEL_OFF4(3))                         \
                RF_G4_PART2(tp[0], gg[1], )                                                         \
            }                                                                                       \
            {                                                                                       \
                P1(3, gg[1], gg[0], ta, 0, 0)                                                       \
                wa_addr -= 16;                                                                      \
                RF_LOAD_WINDOW(wa_addr)                                                             \
                RF_G4_PART2(tp[0], gg[0], RF_COMMA_W)                                               \
            }                                                                                       \
            ta += 4;                                                                                \
        }                                                                                           \
        {                                                                                           \
            float wv[8];                                                                            \
            wv[0] = wna.x; wv[1] = wna.y; wv[2] = wna.z; wv[3] = wna.w;                             \
            wv[4] = wnb.x; wv[5] = wnb.y; wv[6] = wnb.z; wv[7] = wnb.w;                             \
            {                                                                                       \
                P1(0, gg[0], gg[1], ta, RF_TEXEL_OFF4(0), RF_TEXEL_OFF4(1))                         \
                RF_G4_PART2(tp[1], gg[1], )                                                         \
            }                                                                                       \
            {                                                                                       \
                P1(1, gg[1], gg[0], ta, 0, 0)                                                       \
                RF_G4_PART2(tp[1], gg[0], )                                                         \
            }                                                                                       \
            {                                                                                       \
                P1(2, gg[0], gg[1], ta_next, 0, Q4 * 4)                                             \
                RF_G4_PART2(tp[0], gg[1], )                                                         \
            }                                                                                       \
            {                                                                                       \
                P1(3, gg[1], gg[0], ta_next, 0, 0)                                                  \
                RF_LOAD_WINDOW(wa_next)                                                             \
                RF_G4_PART2(tp[0], gg[0], RF_COMMA_W)                                               \
            }                                                                                       \
        }                                                                                           \
        ta = ta_next;                                                                               \
        wa_addr = wa_next;                                                                          \
        ngroups = ngroups_next;                                                                     \
    }
    // (per tap row: all groups but the last run the plain steps; in the last group the two
    //  look-ahead reads fetch columns 0 and 1 of the NEXT row - the columns past the end of this
    //  one carry no weight - step 3 issues that row's first gathers and loads its first weight
    //  window, so the next row starts with a full pipe.  The last row prefetches itself again.)
    if constexpr (J1) {
        RF_ROW_LOOP(RF_G4_PART1_J1)
    } else {
        RF_ROW_LOOP(RF_G4_PART1)
    }
#undef RF_ROW_LOOP
#undef RF_G4_PART1_J1
#undef RF_LOAD_WINDOW
#undef RF_COMMA_W
#undef RF_G4_PART1
#undef RF_G4_PART2
#undef RF_TEXEL_OFF4
#undef RF_TQ
#undef RF_G4_READ
#undef RF_G4_READ_0
#undef RF_G4_READ_1
#undef RF_G4_READ_2
#undef RF_G4_READ_3
#undef RF_G4_TNOUT
#undef RF_G4_TNOUT_0
#undef RF_G4_TNOUT_1
#undef RF_G4_TNOUT_2
#undef RF_G4_TNOUT_3
}

// Which form of the SAD a wave's tap loop takes (jbf_tap_loop_grey4_la2 / jbf_tap_loop_rgb6, MSAD): the
// masked SAD serves a wave only if no lane of it owns a centre with a zero among its joint bytes 0..2
// (v_msad_u8 would leave that channel's difference out).  Known before the loop, reduced over the wave:
// the result is wave-uniform, the branch on it a scalar one.  A lane outside EXEC has no say, and
// neither has one the caller says runs no tap loop (`counts` false: the slab kernel asks with all its
// lanes, those beyond its rows hold a clamped centre).
__device__ __forceinline__ bool jbf_wave_takes_msad(const uint32_t (&jc)[kPix], bool counts = true)
{
    uint32_t z = 0u;
#pragma unroll
    for (int p = 0; p < kPix; p++) {
        const uint32_t v = jc[p] | 0xff000000u;
        z |= (v - 0x01010101u) & ~v & 0x80808080u;  // bit 7 of a byte set <=> one of v's bytes is zero
    }
    return __ballot(counts && z != 0u) == 0ull;
}

// jbf_tap_loop_grey4 with the gathers TWO column steps ahead of their use (round 5).  In the form above
// a column's four LUT gathers are issued in the step before the one that multiplies by them, and the
// step ends in s_waitcnt lgkmcnt(0): a wave has 8 instructions of its own between issue and wait, the
// rest of the LDS latency has to come from the SIMD's other three waves - with the CU's one LDS pipeline
// 62 % busy that is not enough, and VALU and LDS each sit at 0.68 of their floors.  Here step c issues
// the gathers of column c + 2 and waits with lgkmcnt(4): everything but those four gathers - i.e. the
// gathers of column c + 1, the texel pair and the weight window - has landed (LDS operations of a wave
// return in order, so the window is issued BEFORE the step's gathers).  Four gather buffers (indexed by
// the step within the group), the src byte converted when its texel is at hand for the SAD (two steps
// before use) so that a texel pair is free for re-use after its second SAD: two pairs still suffice.
// Same instructions per step, same arithmetic and order: identical bytes.
// The loop runs two groups of four steps per iteration, the two weight windows in two SGPR octets that swap
// roles from group to group (RF_L2_ROW_LOOP): no hand-over, one scalar offset for the window loads.
// SLAB (round 6, jbf_slab_kernel): the loop runs the tap rows i_first .. i_last only - a slab of the disk's
// rows whose texels are what the LDS tile holds at the moment, tile row of tap row i for the lane's output
// row = ty + i + row_bias - and ADDS to sum / wsum: slabs taken in increasing i keep every pixel's taps in
// row-major order, so any radius runs through this loop with the bytes of one pass over the whole disk.
// MSAD (3-channel joint only, never with J1): the SADs are v_msad_u8 with the tap texel as S0 and the
// centre as the reference S1 - the hardware leaves out the bytes whose REFERENCE byte is zero, and byte 3
// of every jc[] is - so the tap texel goes in unmasked: no v_and_b32, no mask register, 25 instead of 26
// VALU instructions per step.  A zero in one of the centre's own channels would drop that channel's
// difference too: the caller picks this form per wave, only where no lane of the wave has such a centre
// (jbf_wave_takes_msad), and the form with the mask otherwise.  Identical bytes.
template <int LUTREP, int TLW, bool J1 = false, bool SLAB = false, bool MSAD = false>
__device__ __forceinline__ void jbf_tap_loop_grey4_la2(uint32_t lut_lane_addr,
                                                       const float *__restrict__ swsym,
                                                       uint32_t tile_lane_addr,
                                                       const uint32_t (&jc)[kPix], int ty, int radius,
                                                       int r4, int sw_len,
                                                       const int *__restrict__ hwtab,
                                                       float (&sum)[kPix][1], float (&wsum)[kPix],
                                                       int i_first = 0, int i_last = 0, int row_bias = 0)
{
    const int i_lo = SLAB ? i_first : -radius, i_hi = SLAB ? i_last : radius;
    const int bias = SLAB ? row_bias : radius;
    constexpr int Q4 = TLW / 4;
    constexpr int SHIFT = LUTREP == 32 ? 7 : LUTREP == 16 ? 6 : LUTREP == 8 ? 5 : 4;
    static_assert(LUTREP == 32 || LUTREP == 16 || LUTREP == 8 || LUTREP == 4, "LUT replicas");
    static_assert(Q4 + 2 <= 255, "ds_read2_b32 offsets are 8 bits (the largest one here: Q4 + 2)");
    static_assert(TLW % 4 == 0, "column-interleaved planes");
    static_assert(!(MSAD && J1), "the single-channel form has no masked SAD");
    [[maybe_unused]] uint32_t mask = 0x00ffffffu;
    if constexpr (!MSAD)
        asm volatile("" : "+v"(mask));  // keep the mask in a VGPR (a literal operand is full-pipe)

    // A tap row of half-width hw serves the lane's four outputs from the 2 hw + 4 columns -hw .. hw + 3.
    // The row starts at the EVEN column -hws (hws = hw rounded up to even) and runs whole groups of four
    // from there: at most two columns of zero weight per row (round 4 started at a multiple of four, the
    // alignment its ds_read_b128 weight windows needed: up to six; 3,664 column steps instead of 3,764
    // per output quad at radius 33).  A row that starts in the middle of a quad of the column-
    // interleaved tile (phase 1) finds columns (0, 1) of a group in planes 2, 3 and columns (2, 3) in
    // planes 0, 1 of the next quad: each of the two pair reads has its own address register.
    const uint32_t lane_row0 = tile_lane_addr + (uint32_t)(ty * TLW * 4);  // the lane's part of an address
    auto row_addr = [&](int i, int hw, uint32_t &ta_out, uint32_t &tb_out, uint32_t &wa_out,
                        int &ngroups_out) {
        const int hws = (hw + 1) & ~1;
        const int ai = i < 0 ? -i : i;
        const int c0 = r4 - hws;  // first column, relative to the lane's quad origin
        const int quad = (i + bias) * TLW + (c0 >> 2);
        const int phase = (c0 >> 1) & 1;
        ta_out = lane_row0 + (uint32_t)((quad + (phase ? 2 * Q4 : 0)) * 4);
        tb_out = lane_row0 + (uint32_t)((quad + (phase ? 1 : 2 * Q4)) * 4);
        // (>= r4 + 4 >= 8, and the row's last window starts at float r4 + 3 - hw >= 4 of the table row: the pair
        //  loop's byte offset `woff` = 4 * index - 32 is never below 0 where a load uses it, see RF_L2_ROW_LOOP;
        //  a table layout with less than 8 floats in front of a row's first window would break that)
        wa_out = (uint32_t)(ai * sw_len + (r4 + 8) + hws - 4);  // index of the first window's first weight
        ngroups_out = (hws + hw + 4 + 3) >> 2;
    };

    uint2v tp[2];        // texel pairs: tp[0] = columns (0, 1), tp[1] = columns (2, 3) of a group
    // The weight window of a group (8 wave-uniform floats) lives in SGPRs: a v_mul_f32 with an SGPR
    // operand hides behind its neighbours like the SADs do (a pair with a v_sad_u8 or a v_add_f32 issues
    // in 4.2 cycles, tools/microbench/pipe_overlap.hip), and two broadcast ds_read_b128 per group - 2 of
    // the 7 dwords an LDS return carried per step, 5 % of the launch - are gone.  Scalar loads share
    // lgkmcnt with the LDS and return out of order, so the window of the NEXT group, requested in step 0,
    // needs a full wait: RF_L2_MID3, placed where it is free.
    typedef float float8v __attribute__((ext_vector_type(8)));
    float8v w8a, w8b;    // the window of this group and that of the next one, in turns (RF_L2_ROW_LOOP)
    float gg[4][kPix];   // gg[u]: LUT values of the group's column u (in flight, then consumed at step u)
    float sv[4];         // sv[u]: src value of column u as float
    uint32_t ta, tb, wa_addr;
    int ngroups;
    int odd = 0;         // the parity of the current row's half-width (wave-uniform; RF_L2_ROW_LOOP)
    if constexpr (SLAB) {
        int hw0;
        const int *hp0 = hwtab + (i_lo + radius);
        asm volatile("s_load_dword %0, %1, 0x0\n\ts_waitcnt lgkmcnt(0)" : "=s"(hw0) : "s"(hp0));
        hw0 = __builtin_amdgcn_readfirstlane(hw0);
        odd = hw0 & 1;
        row_addr(i_lo, hw0, ta, tb, wa_addr, ngroups);
    } else {
        row_addr(-radius, 0, ta, tb, wa_addr, ngroups);  // (the top row of the disk: half-width 0)
    }
    // The half-width of row i + 1 is needed during row i (its last group reads ahead into row i + 1).
    // A load the compiler issues gets its wait - a full one - at the first use, in the middle of a row
    // with four gathers in flight: one pipeline drain per row.  So the value is requested a row early
    // by hand (hw_ahead, at the top of row i - 1) and taken over for row i by the last group of row i - 1,
    // behind the full wait that every group has in the middle of its step 3 (hw_cur: an s_mov inside that
    // statement - a copy the compiler places at the row top instead reads a register whose load is still
    // in flight along the path of the control-flow graph that skips both forms of the last group, which no
    // wave takes and the machine-code check of tests/test_cabi.py walks all the same).
    int hw_ahead, hw_cur;
    {
        const int *hp = SLAB ? hwtab + ((i_lo + 1 < i_hi ? i_lo + 1 : i_hi) + radius) : hwtab + 1;
        asm volatile("s_load_dword %0, %1, 0x0" : "=s"(hw_ahead) : "s"(hp));  // (waited for below)
    }
    // prologue: both texel pairs and the weight window of the first group, gathers and src values of
    // its columns 0 and 1
    asm volatile("ds_read2_b32 %0, %2 offset1:%4\n\t"
                 "ds_read2_b32 %1, %3 offset1:%4"
                 : "=&v"(tp[0]), "=&v"(tp[1])
                 : "v"(ta), "v"(tb), "n"(Q4));
    {
        const float *wp = swsym + wa_addr;
        asm volatile("s_load_dwordx8 %0, %2, 0x0" : "=&s"(w8a), "=s"(w8b) : "s"(wp));  // (w8b: only defined)
    }
    asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(tp[0]), "+v"(tp[1]), "+s"(w8a), "+s"(w8b));
#pragma unroll
    for (int c = 0; c < 2; c++) {
        const uint32_t tx = c == 0 ? tp[0].x : tp[0].y;
        const uint32_t tj = MSAD ? tx : tx & mask;
#pragma unroll
        for (int p = 0; p < kPix; p++) {
            const uint32_t a =
                J1     ? (tj > jc[p] ? tj - jc[p] : jc[p] - tj) + lut_lane_addr
                : MSAD ? __builtin_amdgcn_msad_u8(tj, jc[p], 0u) * (LUTREP * 4u) + lut_lane_addr
                       : __builtin_amdgcn_sad_u8(tj, jc[p], 0u) * (LUTREP * 4u) + lut_lane_addr;
            asm volatile("ds_read_b32 %0, %1" : "=v"(gg[c][p]) : "v"(a));
        }
        sv[c] = (float)(tx >> 24);
    }
    // (the statements of the loop name every gather register and src value as in-out operands: those of
    //  columns 2 and 3 are defined here, without an instruction)
    asm volatile("s_waitcnt lgkmcnt(0)\n\t"
                 "s_mov_b32 %[hwc], %[hwa]"
                 : "+v"(gg[0][0]), "+v"(gg[0][1]), "+v"(gg[0][2]), "+v"(gg[0][3]), "+v"(gg[1][0]),
                   "+v"(gg[1][1]), "+v"(gg[1][2]), "+v"(gg[1][3]), "=v"(gg[2][0]), "=v"(gg[2][1]),
                   "=v"(gg[2][2]), "=v"(gg[2][3]), "=v"(gg[3][0]), "=v"(gg[3][1]), "=v"(gg[3][2]),
                   "=v"(gg[3][3]), "=v"(sv[2]), "=v"(sv[3]), [hwc] "=s"(hw_cur)
                 : [hwa] "s"(hw_ahead));

    // Two column steps - half a group - are ONE statement (hipcc puts an s_nop at every boundary between
    // asm statements that it has nothing else to put at: one statement per step cost 0.5 % against three,
    // round 5).  A half starts with the read of a texel pair of the NEXT group (or of the next row's first
    // group): half 0 its columns (0, 1) into tp[0], half 1 its columns (2, 3) into tp[1] - the pair lands
    // in a 64-bit register whose halves the SADs of the OTHER half take as operands of their own, which is
    // why a whole group cannot be one statement.  Where a pair sits depends on the phase of its row: each
    // of the two reads has its own address register (ta: columns (0, 1), tb: columns (2, 3)), set per row,
    // and the ds_read2 offsets are the same for both phases - no branch in the loop (issuing the read
    // twice under complementary EXEC masks was measured too: the three EXEC writes per read cost more
    // than the shorter rows return).
    // Step X (a: the even one of the half, b: the odd one) of column U: SADs of column U + 2 interleaved
    // with the weights of column U (g: its gathered LUT values); src value of column U + 2; [MID: the
    // group's full wait, step 3]; gather addresses of column U + 2 interleaved with the weight sums of
    // column U; the four gathers (clustered: an LDS instruction between VALU instructions costs their
    // pairing); accumulation of column U (its src value converted two steps ago); the wait that leaves this
    // step's four gathers in flight.  F = AND: the joint bytes of the tap texel masked into tj first;
    // F = MSAD: no such instruction, no tj and no mask operand - the masked SAD takes the texel itself (S0)
    // against the centre (S1); F = J1: one v_sad_u32 forms the table index and the LDS address at once.
#define RF_L2_PRE_AND(X) "v_and_b32 %[tj], %[mask], %[t2" X "]\n\t"
#define RF_L2_PRE_MSAD(X)
#define RF_L2_PRE_J1(X) RF_L2_PRE_AND(X)
#define RF_L2_SAD_AND(X, N) "v_sad_u8 %[a" X #N "], %[tj], %[jc" #N "], 0\n\t"
#define RF_L2_SAD_MSAD(X, N) "v_msad_u8 %[a" X #N "], %[t2" X "], %[jc" #N "], 0\n\t"
#define RF_L2_SAD_J1(X, N) "v_sad_u32 %[a" X #N "], %[tj], %[jc" #N "], %[la]\n\t"
#define RF_L2_ADR_AND(X, N) "v_lshl_add_u32 %[a" X #N "], %[a" X #N "], %[sh], %[la]\n\t"
#define RF_L2_ADR_MSAD(X, N) RF_L2_ADR_AND(X, N)
#define RF_L2_ADR_J1(X, N)
#define RF_L2_TJOUT_AND [tj] "=&v"(tj_),
#define RF_L2_TJOUT_MSAD
#define RF_L2_TJOUT_J1 RF_L2_TJOUT_AND
#define RF_L2_MASKIN_AND [mask] "v"(mask),
#define RF_L2_MASKIN_MSAD
#define RF_L2_MASKIN_J1 RF_L2_MASKIN_AND
#define RF_L2_WMUL(X, N) "v_mul_f32 %[w" #N "], %[wv" X #N "], %[g" X #N "]\n\t"
#define RF_L2_WADD(N) "v_add_f32 %[ws" #N "], %[ws" #N "], %[w" #N "]\n\t"
#define RF_L2_SMUL(X, N) "v_mul_f32 %[w" #N "], %[w" #N "], %[s" X "]\n\t"
#define RF_L2_SADD(N) "v_add_f32 %[s" #N "], %[s" #N "], %[w" #N "]\n\t"
#define RF_L2_GATHER(X, N) "ds_read_b32 %[a" X #N "], %[a" X #N "]\n\t"
    // End groups: a column of a row's first or last group lies outside the disk of some of the lane's four
    // outputs whatever the parity of the half-width - its spatial weight for them is exactly 0, and adding
    // +0.0 to a non-negative sum is the same as not adding it.  A step therefore takes two live masks over
    // the outputs 0..3, FM for its front half (SAD, address and gather of column U + 2) and BM for its back
    // half (the four float instructions of column U), written (o0, o1, o2, o3, number of outputs): a slot's
    // instructions are emitted only where the mask has the output, and the step's wait leaves exactly the
    // gathers it issued in flight.  A back half never runs for a slot whose front half did not (0 x a
    // stale register is not +0 if the register holds an Inf or NaN pattern): BM of column U is a subset of
    // the FM that column's front half was issued with, two steps earlier.
#define RF_L2_M15 (1, 1, 1, 1, 4)
#define RF_L2_M14 (0, 1, 1, 1, 3)
#define RF_L2_M12 (0, 0, 1, 1, 2)
#define RF_L2_M8 (0, 0, 0, 1, 1)
#define RF_L2_M7 (1, 1, 1, 0, 3)
#define RF_L2_M4 (0, 0, 1, 0, 1)
#define RF_L2_M3 (1, 1, 0, 0, 2)
#define RF_L2_M2 (0, 1, 0, 0, 1)
#define RF_L2_M1 (1, 0, 0, 0, 1)
#define RF_L2_M0 (0, 0, 0, 0, 0)
#define RF_L2_SEL0(A, B, C, D, K) A
#define RF_L2_SEL1(A, B, C, D, K) B
#define RF_L2_SEL2(A, B, C, D, K) C
#define RF_L2_SEL3(A, B, C, D, K) D
#define RF_L2_SELK(A, B, C, D, K) K
#define RF_L2_ON_0(T)
#define RF_L2_ON_1(T) T
#define RF_L2_ON_P(B, T) RF_L2_ON_##B(T)
#define RF_L2_ON_E(B, T) RF_L2_ON_P(B, T)
#define RF_L2_ON(M, N, T) RF_L2_ON_E(RF_L2_SEL##N M, T)
#define RF_L2_STR_P(K) #K
#define RF_L2_STR(K) RF_L2_STR_P(K)
#define RF_L2_STEP_TXT(F, X, MID, FM, BM, END)                                                                   \
    RF_L2_PRE_##F(X)                                                                                             \
    RF_L2_ON(FM, 0, RF_L2_SAD_##F(X, 0)) RF_L2_ON(BM, 0, RF_L2_WMUL(X, 0))                                       \
    RF_L2_ON(FM, 1, RF_L2_SAD_##F(X, 1)) RF_L2_ON(BM, 1, RF_L2_WMUL(X, 1))                                       \
    RF_L2_ON(FM, 2, RF_L2_SAD_##F(X, 2)) RF_L2_ON(BM, 2, RF_L2_WMUL(X, 2))                                       \
    RF_L2_ON(FM, 3, RF_L2_SAD_##F(X, 3)) RF_L2_ON(BM, 3, RF_L2_WMUL(X, 3))                                       \
    "v_cvt_f32_ubyte3 %[s2" X "], %[t2" X "]\n\t"                                                                \
    MID                                                                                                          \
    RF_L2_ON(FM, 0, RF_L2_ADR_##F(X, 0)) RF_L2_ON(BM, 0, RF_L2_WADD(0))                                          \
    RF_L2_ON(FM, 1, RF_L2_ADR_##F(X, 1)) RF_L2_ON(BM, 1, RF_L2_WADD(1))                                          \
    RF_L2_ON(FM, 2, RF_L2_ADR_##F(X, 2)) RF_L2_ON(BM, 2, RF_L2_WADD(2))                                          \
    RF_L2_ON(FM, 3, RF_L2_ADR_##F(X, 3)) RF_L2_ON(BM, 3, RF_L2_WADD(3))                                          \
    RF_L2_ON(FM, 0, RF_L2_GATHER(X, 0)) RF_L2_ON(FM, 1, RF_L2_GATHER(X, 1))                                      \
    RF_L2_ON(FM, 2, RF_L2_GATHER(X, 2)) RF_L2_ON(FM, 3, RF_L2_GATHER(X, 3))                                      \
    RF_L2_ON(BM, 0, RF_L2_SMUL(X, 0)) RF_L2_ON(BM, 1, RF_L2_SMUL(X, 1))                                          \
    RF_L2_ON(BM, 2, RF_L2_SMUL(X, 2)) RF_L2_ON(BM, 3, RF_L2_SMUL(X, 3))                                          \
    RF_L2_ON(BM, 0, RF_L2_SADD(0)) RF_L2_ON(BM, 1, RF_L2_SADD(1))                                                \
    RF_L2_ON(BM, 2, RF_L2_SADD(2)) RF_L2_ON(BM, 3, RF_L2_SADD(3))                                                \
    "s_waitcnt lgkmcnt(" RF_L2_STR(RF_L2_SELK FM) ")" END
    // Half H of a group (steps 2 H and 2 H + 1).  WC = the octet that holds the group's window, WN = the
    // one the next group's window is loaded into - both are in-out operands of EVERY statement, so that
    // on every path each of the two C++ variables is only ever the output of a statement of this loop
    // (where an SGPR tuple written by an asm statement meets a value of another origin at a join, the
    // backend merges them in VGPRs and cannot give the result back to an "s" operand).  Half 0 starts with
    // the load of the next window: a scalar load of 8 floats from the table in global memory (scalar
    // cache), address = table + WOFF (an SGPR byte offset) + WIMM.
#define RF_L2_MID3 "s_waitcnt lgkmcnt(0)\n\t"
#define RF_L2_MID3_LAST "s_waitcnt lgkmcnt(0)\n\ts_mov_b32 %[hwc], %[hwa]\n\t"
#define RF_L2_WLOAD_0 "s_load_dwordx8 %[wn], %[wb], %[wo] offset:%[wi]\n\t"
#define RF_L2_WLOAD_1
#define RF_L2_HALF(F, H, WC, WN, TA, O0, O1, WOFF, WIMM, MIDB, FA, BA, FB, BB)                                   \
    {                                                                                                            \
        float w0_, w1_, w2_, w3_;                                                                                \
        [[maybe_unused]] uint32_t tj_;                                                                           \
        asm volatile(RF_L2_WLOAD_##H                                                                             \
                     "ds_read2_b32 %[tn], %[ta] offset0:%[o0] offset1:%[o1]\n\t"                                 \
                     RF_L2_STEP_TXT(F, "a", "", FA, BA, "\n\t")                                                  \
                     RF_L2_STEP_TXT(F, "b", MIDB, FB, BB, "")                                                    \
                     : [tn] "=&v"(tp[H]), RF_L2_TJOUT_##F                                                        \
                       [aa0] "+v"(gg[(2 * (H) + 2) & 3][0]), [aa1] "+v"(gg[(2 * (H) + 2) & 3][1]),               \
                       [aa2] "+v"(gg[(2 * (H) + 2) & 3][2]), [aa3] "+v"(gg[(2 * (H) + 2) & 3][3]),               \
                       [ab0] "+v"(gg[(2 * (H) + 3) & 3][0]), [ab1] "+v"(gg[(2 * (H) + 3) & 3][1]),               \
                       [ab2] "+v"(gg[(2 * (H) + 3) & 3][2]), [ab3] "+v"(gg[(2 * (H) + 3) & 3][3]),               \
                       [ga0] "+v"(gg[2 * (H)][0]), [ga1] "+v"(gg[2 * (H)][1]),                                   \
                       [ga2] "+v"(gg[2 * (H)][2]), [ga3] "+v"(gg[2 * (H)][3]),                                   \
                       [gb0] "+v"(gg[2 * (H) + 1][0]), [gb1] "+v"(gg[2 * (H) + 1][1]),                           \
                       [gb2] "+v"(gg[2 * (H) + 1][2]), [gb3] "+v"(gg[2 * (H) + 1][3]),                           \
                       [w0] "=&v"(w0_), [w1] "=&v"(w1_), [w2] "=&v"(w2_), [w3] "=&v"(w3_),                       \
                       [s2a] "=&v"(sv[(2 * (H) + 2) & 3]), [s2b] "=&v"(sv[(2 * (H) + 3) & 3]),                   \
                       [ws0] "+v"(wsum[0]), [ws1] "+v"(wsum[1]), [ws2] "+v"(wsum[2]),                            \
                       [ws3] "+v"(wsum[3]), [s0] "+v"(sum[0][0]), [s1] "+v"(sum[1][0]),                          \
                       [s2] "+v"(sum[2][0]), [s3] "+v"(sum[3][0]), [wc] "+s"(WC), [wn] "+s"(WN),                 \
                       [hwc] "+s"(hw_cur)                                                                        \
                     : [ta] "v"(TA), [o0] "n"(O0), [o1] "n"(O1), RF_L2_MASKIN_##F                                \
                       [t2a] "v"(tp[1 - (H)][0]), [t2b] "v"(tp[1 - (H)][1]), [jc0] "v"(jc[0]),                   \
                       [jc1] "v"(jc[1]), [jc2] "v"(jc[2]), [jc3] "v"(jc[3]),                                     \
                       [wva0] "s"(WC[4 - 2 * (H)]), [wva1] "s"(WC[5 - 2 * (H)]),                                 \
                       [wva2] "s"(WC[6 - 2 * (H)]), [wva3] "s"(WC[7 - 2 * (H)]),                                 \
                       [wvb0] "s"(WC[3 - 2 * (H)]), [wvb1] "s"(WC[4 - 2 * (H)]),                                 \
                       [wvb2] "s"(WC[5 - 2 * (H)]), [wvb3] "s"(WC[6 - 2 * (H)]),                                 \
                       [sh] "n"(SHIFT), [la] "v"(lut_lane_addr), [sa] "v"(sv[2 * (H)]),                          \
                       [sb] "v"(sv[2 * (H) + 1]), [wb] "s"(swsym), [wo] "s"(WOFF),                               \
                       [wi] "n"(WIMM), [hwa] "s"(hw_ahead));                                                     \
    }
    // (The last step of a row waits like any other: its gathers - two of them, the fronts [3] of the next
    //  row's column 1 - stay in flight across the row loop's
    //  back edge, where the compiler writes code of its own - the next row's addresses.  That it moves
    //  none of the registers in flight there is checked on the machine code, along every path of the
    //  control-flow graph: tests/test_cabi.py.  A variant of this loop once got such a v_mov; a full wait
    //  at the row end, which this loop had until the check walked branches, costs 0.3 %.)
    // One group of four steps; NA / NB = address registers of the texel pairs read ahead (this row's next
    // group or the next row's first one), PA / PB their ds_read2 offsets; the group's full wait - for the
    // weight window requested at its top - sits in the middle of step 3, where nothing is in flight but
    // the gathers of step 2, a whole step old (step 3 reads no texel pair).
    // F0 B0 .. F3 B3: the front and back masks of the group's steps 0..3.
#define RF_L2_GROUP_M(F, WC, WN, NA, NB, PA, PB, WOFF, WIMM, MID3, F0, B0, F1, B1, F2, B2, F3, B3)               \
    RF_L2_HALF(F, 0, WC, WN, NA, PA, PB, WOFF, WIMM, "", F0, B0, F1, B1)                                         \
    RF_L2_HALF(F, 1, WC, WN, NB, PA, PB, WOFF, WIMM, MID3, F2, B2, F3, B3)
#define RF_L2_GROUP(F, WC, WN, NA, NB, PA, PB, WOFF, WIMM, MID3)                                                 \
    RF_L2_GROUP_M(F, WC, WN, NA, NB, PA, PB, WOFF, WIMM, MID3, RF_L2_M15, RF_L2_M15, RF_L2_M15, RF_L2_M15,       \
                  RF_L2_M15, RF_L2_M15, RF_L2_M15, RF_L2_M15)
    // The last group of a row: its columns 0..3 are live for the outputs [15, 14, 12, 8] at most (column u
    // lies right of the disk of every output below u), so the front halves of its own columns 2 and 3 -
    // issued in its steps 0 and 1 - take [12, 8]; steps 2 and 3 form the next row's columns 0 and 1, whose
    // back halves - in that row's first group - take [1, 3].
#define RF_L2_GROUP_LAST(F, WC, WN, NA, NB, PA, PB, WOFF, WIMM)                                                  \
    RF_L2_GROUP_M(F, WC, WN, NA, NB, PA, PB, WOFF, WIMM, RF_L2_MID3_LAST, RF_L2_M12, RF_L2_M15, RF_L2_M8,        \
                  RF_L2_M14, RF_L2_M1, RF_L2_M12, RF_L2_M3, RF_L2_M8)
    // The first group of a row of two groups or more: columns 0..3 live for [1, 3, 7, 15] (column u lies left
    // of the disk of every output above u); the fronts of columns 0 and 1 came from the row before.
#define RF_L2_GROUP_FIRST(F, WC, WN, NA, NB, PA, PB, WOFF, WIMM)                                                 \
    RF_L2_GROUP_M(F, WC, WN, NA, NB, PA, PB, WOFF, WIMM, RF_L2_MID3, RF_L2_M7, RF_L2_M1, RF_L2_M15, RF_L2_M3,    \
                  RF_L2_M15, RF_L2_M7, RF_L2_M15, RF_L2_M15)
    // A row of one group (half-width 0, the disk's top and bottom rows) is first and last at once: the
    // intersection [1, 2, 4, 8] - each output's own column.
#define RF_L2_GROUP_SINGLE(F, WC, WN, NA, NB, PA, PB, WOFF, WIMM)                                                \
    RF_L2_GROUP_M(F, WC, WN, NA, NB, PA, PB, WOFF, WIMM, RF_L2_MID3_LAST, RF_L2_M4, RF_L2_M1, RF_L2_M8,          \
                  RF_L2_M2, RF_L2_M1, RF_L2_M4, RF_L2_M3, RF_L2_M8)
    // Rows of ODD half-width (hws = hw + 1): the row's first column lies left of the disk of all four outputs
    // and the padding column at its end right of it - the live outputs are [0, 1, 3, 7] and [14, 12, 8, 0],
    // one output less per column than the masks above, which are the union over both parities.  The first
    // and the last group of such a row have forms of their own (an odd row has at least two groups): the
    // step of the dead column issues no back half, the step that would form the dead column no gather (it
    // ends in a full wait).  The last group goes on issuing the NEXT row's columns 0 and 1 with [1, 3]
    // whatever that row's parity: the first group of either parity runs a subset of them.
#define RF_L2_GROUP_FIRST_ODD(F, WC, WN, NA, NB, PA, PB, WOFF, WIMM)                                             \
    RF_L2_GROUP_M(F, WC, WN, NA, NB, PA, PB, WOFF, WIMM, RF_L2_MID3, RF_L2_M3, RF_L2_M0, RF_L2_M7, RF_L2_M1,     \
                  RF_L2_M15, RF_L2_M3, RF_L2_M15, RF_L2_M7)
#define RF_L2_GROUP_LAST_ODD(F, WC, WN, NA, NB, PA, PB, WOFF, WIMM)                                              \
    RF_L2_GROUP_M(F, WC, WN, NA, NB, PA, PB, WOFF, WIMM, RF_L2_MID3_LAST, RF_L2_M8, RF_L2_M14, RF_L2_M0,         \
                  RF_L2_M12, RF_L2_M1, RF_L2_M8, RF_L2_M3, RF_L2_M0)
    // The two octets swap roles from group to group: a group in role A multiplies from w8a and loads the
    // next window into w8b, one in role B the other way round - no copy hands the window on.  Which octet
    // holds the current window is a state of the control flow (`in_b`, tested at the row top).  A row of two
    // groups or more runs: its FIRST group in the role it starts in; where that was an A and more groups
    // follow, one lone B group; PAIRS of groups, A then B; a lone A group where one is left over; and its
    // LAST group - the one that reads ahead into the next row through ta_next / tb_next and loads its first
    // window -, which exists in both roles, so rows with an odd number of groups need neither a padding
    // group nor a copy and the next row simply starts in the other role.  A row of one group runs the SINGLE
    // form in its role.  Inside a pair the second group's ds_read2 offsets are the first group's plus one
    // dword and ta / tb advance once, by 8 bytes; a lone group advances them by 4.  The windows of a row
    // descend by 16 bytes per group: woff = byte offset of the current window - 32, one s_sub per pair or
    // lone group; the loads take woff + 16 and woff + 0 (never below 0 where used: a row's last window
    // starts at float r4 + 3 - hw >= 4 of its table row).
#define RF_L2_ROW_LOOP(F)                                                                                        \
    for (int i = i_lo; i <= i_hi; i++) {                                                                         \
        uint32_t ta_next, tb_next, wa_next;                                                                      \
        int ngroups_next;                                                                                        \
        row_addr(i < i_hi ? i + 1 : i, __builtin_amdgcn_readfirstlane(hw_cur), ta_next,                          \
                 tb_next, wa_next, ngroups_next);                                                                \
        {                                                                                                        \
            const int *hp_ = hwtab + ((i + 2 < i_hi ? i + 2 : i_hi) + radius);                                   \
            /* (in-out: the register stays hw_ahead's from row to row - a register that is free at               \
                the row top the compiler takes for that row's address arithmetic, and the machine-code           \
                check sees the load of the row before still in flight there along the path that skips            \
                both forms of the last group) */                                                                 \
            asm volatile("s_load_dword %0, %1, 0x0" : "+s"(hw_ahead) : "s"(hp_));                                \
        }                                                                                                        \
        const uint32_t woff_next = wa_next * 4u;                                                                 \
        int m = ngroups - 1; /* groups before the row's last one */                                              \
        /* (hw_cur is the NEXT row's half-width until this row's last group takes over the one after) */        \
        const int odd_next = __builtin_amdgcn_readfirstlane(hw_cur) & 1;                                         \
        /* the row's first group: role A or B, even or odd half-width - four alternative ifs in sequence on a    \
            value built without a compare (m > 0 as min(m, 1), an s_min: a compare result lives in VCC and does  \
            not pass an empty asm statement, "illegal VGPR to SGPR copy", and the sign bit of -m is turned back  \
            into one), each but the first behind the barrier of the closing forms below.  fsel 0: a row of one   \
            group has no first group */                                                                          \
        int has_first = m < 1 ? m : 1;                                                                           \
        asm volatile("" : "+s"(has_first)); /* (a number from here on, not a condition) */                       \
        int fsel = (1 + in_b + 2 * odd) & -has_first;                                                            \
        if (fsel == 1) {                                                                                         \
            RF_L2_GROUP_FIRST(F, w8a, w8b, ta, tb, 1, Q4 + 1, woff, 16)                                          \
        }                                                                                                        \
        asm volatile("" : "+s"(fsel));                                                                           \
        fsel = __builtin_amdgcn_readfirstlane(fsel);                                                             \
        if (fsel == 2) {                                                                                         \
            RF_L2_GROUP_FIRST(F, w8b, w8a, ta, tb, 1, Q4 + 1, woff, 16)                                          \
        }                                                                                                        \
        asm volatile("" : "+s"(fsel));                                                                           \
        fsel = __builtin_amdgcn_readfirstlane(fsel);                                                             \
        if (fsel == 3) {                                                                                         \
            RF_L2_GROUP_FIRST_ODD(F, w8a, w8b, ta, tb, 1, Q4 + 1, woff, 16)                                      \
        }                                                                                                        \
        asm volatile("" : "+s"(fsel));                                                                           \
        fsel = __builtin_amdgcn_readfirstlane(fsel);                                                             \
        if (fsel == 4) {                                                                                         \
            RF_L2_GROUP_FIRST_ODD(F, w8b, w8a, ta, tb, 1, Q4 + 1, woff, 16)                                      \
        }                                                                                                        \
        /* what a first group leaves behind, without a branch: the addresses one group on, and the remaining    \
            groups start in the other role (lone_b: they start in B) */                                          \
        ta += 4 * has_first;                                                                                     \
        tb += 4 * has_first;                                                                                     \
        woff -= 16 * has_first;                                                                                  \
        m -= has_first;                                                                                          \
        int lone_b = in_b ^ has_first;                                                                           \
        const int mid_b = lone_b & (int)(m > 0); /* (a row of one group has m == 0) */                           \
        if (mid_b) {                                                                                             \
            RF_L2_GROUP(F, w8b, w8a, ta, tb, 1, Q4 + 1, woff, 16, RF_L2_MID3)                                    \
            ta += 4;                                                                                             \
            tb += 4;                                                                                             \
            woff -= 16;                                                                                          \
            m--;                                                                                                 \
            lone_b = 0;                                                                                          \
        }                                                                                                        \
        for (int k = m >> 1; k > 0; k--) {                                                                       \
            RF_L2_GROUP(F, w8a, w8b, ta, tb, 1, Q4 + 1, woff, 16, RF_L2_MID3)                                    \
            RF_L2_GROUP(F, w8b, w8a, ta, tb, 2, Q4 + 2, woff, 0, RF_L2_MID3)                                     \
            ta += 8;                                                                                             \
            tb += 8;                                                                                             \
            woff -= 32;                                                                                          \
        }                                                                                                        \
        if (m & 1) {                                                                                             \
            RF_L2_GROUP(F, w8a, w8b, ta, tb, 1, Q4 + 1, woff, 16, RF_L2_MID3)                                    \
        }                                                                                                        \
        /* the row's closing group: last, single or last of an odd row, role A or B - six alternative ifs in     \
            sequence, each but the first on a value the compiler cannot see through: an if / else with a         \
            statement of this loop in either arm is structurized into two ifs with the state BEFORE the first    \
            arm kept alive for the second, which costs a copy of every register of the loop */                   \
        const int last_a = ((lone_b | m) & 1) ^ 1;                                                               \
        int sel = last_a | ((int)(ngroups == 1) << 1) | (odd << 2); /* (an odd row is never a single) */         \
        if (sel == 0) {                                                                                          \
            RF_L2_GROUP_LAST(F, w8b, w8a, ta_next, tb_next, 0, Q4, woff_next, 0)                                 \
        }                                                                                                        \
        asm volatile("" : "+s"(sel));                                                                            \
        sel = __builtin_amdgcn_readfirstlane(sel);                                                               \
        if (sel == 1) {                                                                                          \
            RF_L2_GROUP_LAST(F, w8a, w8b, ta_next, tb_next, 0, Q4, woff_next, 0)                                 \
        }                                                                                                        \
        asm volatile("" : "+s"(sel));                                                                            \
        sel = __builtin_amdgcn_readfirstlane(sel);                                                               \
        if (sel == 2) {                                                                                          \
            RF_L2_GROUP_SINGLE(F, w8b, w8a, ta_next, tb_next, 0, Q4, woff_next, 0)                               \
        }                                                                                                        \
        asm volatile("" : "+s"(sel));                                                                            \
        sel = __builtin_amdgcn_readfirstlane(sel);                                                               \
        if (sel == 3) {                                                                                          \
            RF_L2_GROUP_SINGLE(F, w8a, w8b, ta_next, tb_next, 0, Q4, woff_next, 0)                               \
        }                                                                                                        \
        asm volatile("" : "+s"(sel));                                                                            \
        sel = __builtin_amdgcn_readfirstlane(sel);                                                               \
        if (sel == 4) {                                                                                          \
            RF_L2_GROUP_LAST_ODD(F, w8b, w8a, ta_next, tb_next, 0, Q4, woff_next, 0)                             \
        }                                                                                                        \
        asm volatile("" : "+s"(sel));                                                                            \
        sel = __builtin_amdgcn_readfirstlane(sel);                                                               \
        if (sel == 5) {                                                                                          \
            RF_L2_GROUP_LAST_ODD(F, w8a, w8b, ta_next, tb_next, 0, Q4, woff_next, 0)                             \
        }                                                                                                        \
        in_b = sel & 1;                                                                                          \
        odd = odd_next;                                                                                          \
        ta = ta_next;                                                                                            \
        tb = tb_next;                                                                                            \
        woff = woff_next - 32u;                                                                                  \
        ngroups = ngroups_next;                                                                                  \
    }
    int in_b = 0;  // the prologue loaded the first window into w8a
    uint32_t woff = wa_addr * 4u - 32u;
    if constexpr (J1) {
        RF_L2_ROW_LOOP(J1)
    } else if constexpr (MSAD) {
        RF_L2_ROW_LOOP(MSAD)
    } else {
        RF_L2_ROW_LOOP(AND)
    }
    // the last steps' gathers (of a row that does not exist) are still in flight: nothing may re-use
    // their registers before they have landed
    asm volatile("s_waitcnt lgkmcnt(0)"
                 : "+v"(gg[0][0]), "+v"(gg[0][1]), "+v"(gg[0][2]), "+v"(gg[0][3]), "+v"(gg[1][0]),
                   "+v"(gg[1][1]), "+v"(gg[1][2]), "+v"(gg[1][3]), "+v"(tp[0]), "+v"(tp[1]),
                   "+s"(w8a), "+s"(w8b), "+s"(hw_ahead));
#undef RF_L2_ROW_LOOP
#undef RF_L2_GROUP_SINGLE
#undef RF_L2_GROUP_FIRST
#undef RF_L2_GROUP_LAST
#undef RF_L2_GROUP
#undef RF_L2_GROUP_M
#undef RF_L2_HALF
#undef RF_L2_WLOAD_0
#undef RF_L2_MID3
#undef RF_L2_MID3_LAST
#undef RF_L2_WLOAD_1
#undef RF_L2_STEP_TXT
    // (the live masks RF_L2_M* and RF_L2_ON stay defined for jbf_tap_loop_rgb6 below)
#undef RF_L2_GROUP_LAST_ODD
#undef RF_L2_GROUP_FIRST_ODD
#undef RF_L2_GATHER
#undef RF_L2_SADD
#undef RF_L2_SMUL
#undef RF_L2_WADD
#undef RF_L2_WMUL
#undef RF_L2_MASKIN_J1
#undef RF_L2_MASKIN_MSAD
#undef RF_L2_MASKIN_AND
#undef RF_L2_TJOUT_J1
#undef RF_L2_TJOUT_MSAD
#undef RF_L2_TJOUT_AND
#undef RF_L2_ADR_J1
#undef RF_L2_ADR_MSAD
#undef RF_L2_ADR_AND
#undef RF_L2_SAD_J1
#undef RF_L2_SAD_MSAD
#undef RF_L2_SAD_AND
#undef RF_L2_PRE_J1
#undef RF_L2_PRE_MSAD
#undef RF_L2_PRE_AND
}

// Hand-scheduled tap loop for colour tiles with 6-byte texels (main plane {B,G,R joint, B src},
// second plane {G src, R src}): the arithmetic and the pipeline of jbf_tap_loop<3, LUTREP, false,
// TLW, 6>, the row-carried prologue of jbf_tap_loop_grey4.  Per column step 44 VALU instructions,
// 12 of them on the full pipe (v_and with the literal mask kept in a VGPR is not): 4 v_sad_u8,
// 4 v_lshl_add_u32, 3 v_cvt_f32_ubyte*; hipcc emits the SADs and address computations as one
// burst of nine, here each full-pipe instruction is followed by a simple one (v_mul/v_add).
// SLAB: tap rows i_first .. i_last only, tile row of tap row i = ty + i + row_bias, sums ADDED to (see
// jbf_tap_loop_grey4_la2).
// MSAD: v_msad_u8 on the unmasked tap texel, 43 instructions per step, chosen per wave (see
// jbf_tap_loop_grey4_la2).
template <int LUTREP, int TLW, bool SLAB = false, bool MSAD = false>
__device__ __forceinline__ void jbf_tap_loop_rgb6(uint32_t lut_lane_addr,
                                                  const float *__restrict__ swsym,
                                                  uint32_t tile_lane_addr,
                                                  uint32_t plane_b_lane_addr,
                                                  const uint32_t (&jc)[kPix], int ty, int radius,
                                                  int r4, int sw_len,
                                                  const int *__restrict__ hwtab,
                                                  float (&sum)[kPix][3], float (&wsum)[kPix],
                                                  int i_first = 0, int i_last = 0, int row_bias = 0)
{
    const int i_lo = SLAB ? i_first : -radius, i_hi = SLAB ? i_last : radius;
    const int bias = SLAB ? row_bias : radius;
    constexpr int Q4 = TLW / 4;
    constexpr int SHIFT = LUTREP == 32 ? 7 : LUTREP == 16 ? 6 : LUTREP == 8 ? 5 : 4;
    static_assert(LUTREP == 32 || LUTREP == 16 || LUTREP == 8 || LUTREP == 4, "LUT replicas");
    [[maybe_unused]] uint32_t mask = 0x00ffffffu;
    if constexpr (!MSAD)
        asm volatile("" : "+v"(mask));  // keep the mask in a VGPR (a literal operand is full-pipe)

    // Rows start at the even column -hws and run whole groups of four, as in jbf_tap_loop_grey4_la2.
    // Steps 0, 1 of a group read columns 2, 3 of the group through the address pair (ta, tb), steps 2, 3
    // read columns 0, 1 of the NEXT group through (ta2, tb2) - the row's phase decides which planes of
    // the column-interleaved tile those are, the offsets in the instructions do not change.
    auto row_addr = [&](int i, uint32_t &ta_out, uint32_t &tb_out, uint32_t &ta2_out,
                        uint32_t &tb2_out, uint32_t &wa_out, int &ngroups_out) {
        const int hw = hwtab[i + radius];
        const int hws = (hw + 1) & ~1;
        const int ai = i < 0 ? -i : i;
        const int c0 = r4 - hws;  // first column, relative to the lane's quad origin
        const uint32_t quad = (uint32_t)((ty + i + bias) * TLW + (c0 >> 2));
        const bool phase = ((c0 >> 1) & 1) != 0;
        const uint32_t q23 = quad + (phase ? 1u : 2u * Q4);  // columns 2, 3 of the row's first group
        const uint32_t q01 = quad + (phase ? 2u * Q4 : 0u);  // columns 0, 1 of the row's first group
        ta_out = tile_lane_addr + q23 * 4;
        tb_out = plane_b_lane_addr + q23 * 2;
        ta2_out = tile_lane_addr + q01 * 4;
        tb2_out = plane_b_lane_addr + q01 * 2;
        wa_out = (uint32_t)(ai * sw_len + (r4 + 8) + hws - 4);  // index of the first window's first weight
        ngroups_out = (hws + hw + 4 + 3) >> 2;
    };

    uint32_t tq[4], tqb[4];
    // the weight window of a group in SGPRs, as in jbf_tap_loop_grey4_la2: every step ends with a full
    // wait here, so the scalar load of the next window (issued in step 3, after that step's gathers)
    // needs no wait of its own
    typedef float float8v __attribute__((ext_vector_type(8)));
    float8v ws8, wn8;
    float gg[2][kPix];
    uint32_t ta, tb, ta2, tb2, wa_addr;
    int ngroups;
    row_addr(i_lo, ta, tb, ta2, tb2, wa_addr, ngroups);
    // prologue of the first tap row (later rows get theirs from the last group of the row before)
    asm volatile("ds_read_b32 %0, %4\n\t"
                 "ds_read_b32 %1, %4 offset:%6\n\t"
                 "ds_read_u16 %2, %5\n\t"
                 "ds_read_u16 %3, %5 offset:%7"
                 : "=&v"(tq[0]), "=&v"(tq[1]), "=&v"(tqb[0]), "=&v"(tqb[1])
                 : "v"(ta2), "v"(tb2), "n"(Q4 * 4), "n"(Q4 * 2));
    {
        const float *wp = swsym + wa_addr;
        asm volatile("s_load_dwordx8 %0, %1, 0x0" : "=&s"(ws8) : "s"(wp));
    }
    // (a scalar load returns out of order: the first texel needs a full wait as well)
    asm volatile("s_waitcnt lgkmcnt(0)"
                 : "+v"(tq[0]), "+v"(tq[1]), "+v"(tqb[0]), "+v"(tqb[1]), "+s"(ws8));
    {
        const uint32_t tj = MSAD ? tq[0] : tq[0] & mask;
#pragma unroll
        for (int p = 0; p < kPix; p++) {
            const uint32_t a = (MSAD ? __builtin_amdgcn_msad_u8(tj, jc[p], 0u)
                                     : __builtin_amdgcn_sad_u8(tj, jc[p], 0u)) * (LUTREP * 4u) +
                               lut_lane_addr;
            asm volatile("ds_read_b32 %0, %1" : "=v"(gg[0][p]) : "v"(a));
        }
    }
    asm volatile("s_waitcnt lgkmcnt(0)"
                 : "+v"(gg[0][0]), "+v"(gg[0][1]), "+v"(gg[0][2]), "+v"(gg[0][3]));

    // Column step U: texel (both planes) of column +2 from TA/TB + offset, SAD + gathers of column
    // +1, accumulation of column +0.  GA = gathers consumed, GB = gathers issued (their registers
    // hold alpha, then the LDS address, then the LUT value).
    // F = AND: v_and_b32 into tj, then v_sad_u8 on tj; F = MSAD: v_msad_u8 on the texel itself.
#define RF_C6_AND_AND "v_and_b32 %[tj], %[mask], %[t1]\n\t"
#define RF_C6_AND_MSAD
#define RF_C6_TJOUT_AND [tj] "=&v"(tj_),
#define RF_C6_TJOUT_MSAD
#define RF_C6_MASKIN_AND [mask] "v"(mask),
#define RF_C6_MASKIN_MSAD
#define RF_C6_SAD_AND(N) "v_sad_u8 %[a" #N "], %[tj], %[jc" #N "], 0\n\t"
#define RF_C6_SAD_MSAD(N) "v_msad_u8 %[a" #N "], %[t1], %[jc" #N "], 0\n\t"
    // End groups, as in jbf_tap_loop_grey4_la2: FM = live outputs of the step's front half (SAD, address and
    // gather of column U + 1), BM = those of its back half (the eight float instructions of column U); the
    // texel reads, the three conversions and the step's full wait are not slots.  BM of a column is a subset
    // of the FM its front half was issued with, one step earlier.
#define RF_C6_WMUL(N) "v_mul_f32 %[w" #N "], %[wv" #N "], %[g" #N "]\n\t"
#define RF_C6_WADD(N) "v_add_f32 %[ws" #N "], %[ws" #N "], %[w" #N "]\n\t"
#define RF_C6_ADR(N) "v_lshl_add_u32 %[a" #N "], %[a" #N "], %[sh], %[la]\n\t"
#define RF_C6_GATHER(N) "ds_read_b32 %[a" #N "], %[a" #N "]\n\t"
#define RF_C6_CMUL(N, C) "v_mul_f32 %[m" #N "], %[w" #N "], %[s" #C "]\n\t"
#define RF_C6_CADD(N, C) "v_add_f32 %[c" #N #C "], %[c" #N #C "], %[m" #N "]\n\t"
#define RF_C6_CH(BM, C)                                                                          \
    RF_L2_ON(BM, 0, RF_C6_CMUL(0, C)) RF_L2_ON(BM, 1, RF_C6_CMUL(1, C))                          \
    RF_L2_ON(BM, 2, RF_C6_CMUL(2, C)) RF_L2_ON(BM, 3, RF_C6_CMUL(3, C))                          \
    RF_L2_ON(BM, 0, RF_C6_CADD(0, C)) RF_L2_ON(BM, 1, RF_C6_CADD(1, C))                          \
    RF_L2_ON(BM, 2, RF_C6_CADD(2, C)) RF_L2_ON(BM, 3, RF_C6_CADD(3, C))
#define RF_C6_STEP(F, U, GA, GB, TA, TB, OFFT, EXTRA_ASM, EXTRA_OPERANDS, FM, BM)                \
    {                                                                                            \
        float w0_, w1_, w2_, w3_, s0_, s1_, s2_, m0_, m1_, m2_, m3_;                             \
        [[maybe_unused]] uint32_t tj_;                                                           \
        EXTRA_ASM /* (step 3: the next window's scalar load; the step ends in a full wait) */    \
        asm volatile("ds_read_b32 %[tn], %[ta] offset:%[off4]\n\t"                               \
                     "ds_read_u16 %[tnb], %[tb] offset:%[off2]\n\t"                              \
                     RF_C6_AND_##F                                                               \
                     RF_L2_ON(FM, 0, RF_C6_SAD_##F(0)) RF_L2_ON(BM, 0, RF_C6_WMUL(0))            \
                     RF_L2_ON(FM, 1, RF_C6_SAD_##F(1)) RF_L2_ON(BM, 1, RF_C6_WMUL(1))            \
                     RF_L2_ON(FM, 2, RF_C6_SAD_##F(2)) RF_L2_ON(BM, 2, RF_C6_WMUL(2))            \
                     RF_L2_ON(FM, 3, RF_C6_SAD_##F(3)) RF_L2_ON(BM, 3, RF_C6_WMUL(3))            \
                     "v_cvt_f32_ubyte3 %[s0], %[t0]\n\t"                                         \
                     RF_L2_ON(BM, 0, RF_C6_WADD(0))                                              \
                     "v_cvt_f32_ubyte0 %[s1], %[tb0]\n\t"                                        \
                     RF_L2_ON(BM, 1, RF_C6_WADD(1))                                              \
                     "v_cvt_f32_ubyte1 %[s2], %[tb0]\n\t"                                        \
                     RF_L2_ON(BM, 2, RF_C6_WADD(2))                                              \
                     RF_L2_ON(FM, 0, RF_C6_ADR(0)) RF_L2_ON(BM, 3, RF_C6_WADD(3))                \
                     RF_L2_ON(FM, 1, RF_C6_ADR(1)) RF_L2_ON(BM, 0, RF_C6_CMUL(0, 0))             \
                     RF_L2_ON(FM, 2, RF_C6_ADR(2)) RF_L2_ON(BM, 1, RF_C6_CMUL(1, 0))             \
                     RF_L2_ON(FM, 3, RF_C6_ADR(3)) RF_L2_ON(BM, 2, RF_C6_CMUL(2, 0))             \
                     RF_L2_ON(FM, 0, RF_C6_GATHER(0)) RF_L2_ON(FM, 1, RF_C6_GATHER(1))           \
                     RF_L2_ON(FM, 2, RF_C6_GATHER(2)) RF_L2_ON(FM, 3, RF_C6_GATHER(3))           \
                     RF_L2_ON(BM, 3, RF_C6_CMUL(3, 0))                                           \
                     RF_L2_ON(BM, 0, RF_C6_CADD(0, 0)) RF_L2_ON(BM, 1, RF_C6_CADD(1, 0))         \
                     RF_L2_ON(BM, 2, RF_C6_CADD(2, 0)) RF_L2_ON(BM, 3, RF_C6_CADD(3, 0))         \
                     RF_C6_CH(BM, 1)                                                             \
                     RF_C6_CH(BM, 2)                                                             \
                     "s_waitcnt lgkmcnt(0)"                                                      \
                     : [tn] "=&v"(tq[((U) + 2) & 3]), [tnb] "=&v"(tqb[((U) + 2) & 3]),           \
                       RF_C6_TJOUT_##F [a0] "=&v"(GB[0]), [a1] "=&v"(GB[1]), [a2] "=&v"(GB[2]),  \
                       [a3] "=&v"(GB[3]), [w0] "=&v"(w0_), [w1] "=&v"(w1_), [w2] "=&v"(w2_),     \
                       [w3] "=&v"(w3_), [s0] "=&v"(s0_), [s1] "=&v"(s1_), [s2] "=&v"(s2_),       \
                       [m0] "=&v"(m0_), [m1] "=&v"(m1_), [m2] "=&v"(m2_), [m3] "=&v"(m3_),       \
                       [ws0] "+v"(wsum[0]), [ws1] "+v"(wsum[1]), [ws2] "+v"(wsum[2]),            \
                       [ws3] "+v"(wsum[3]),                                                      \
                       [c00] "+v"(sum[0][0]), [c10] "+v"(sum[1][0]), [c20] "+v"(sum[2][0]),      \
                       [c30] "+v"(sum[3][0]), [c01] "+v"(sum[0][1]), [c11] "+v"(sum[1][1]),      \
                       [c21] "+v"(sum[2][1]), [c31] "+v"(sum[3][1]), [c02] "+v"(sum[0][2]),      \
                       [c12] "+v"(sum[1][2]), [c22] "+v"(sum[2][2]), [c32] "+v"(sum[3][2])       \
                       EXTRA_OPERANDS                                                            \
                     : [ta] "v"(TA), [tb] "v"(TB), [off4] "n"((OFFT) * 4), [off2] "n"((OFFT) * 2), \
                       RF_C6_MASKIN_##F [t1] "v"(tq[((U) + 1) & 3]), [t0] "v"(tq[(U)]),          \
                       [tb0] "v"(tqb[(U)]), [jc0] "v"(jc[0]), [jc1] "v"(jc[1]), [jc2] "v"(jc[2]), \
                       [jc3] "v"(jc[3]), [wv0] "s"(wv[4 - (U)]), [wv1] "s"(wv[5 - (U)]),         \
                       [wv2] "s"(wv[6 - (U)]), [wv3] "s"(wv[7 - (U)]), [g0] "v"(GA[0]),          \
                       [g1] "v"(GA[1]), [g2] "v"(GA[2]), [g3] "v"(GA[3]), [sh] "n"(SHIFT),       \
                       [la] "v"(lut_lane_addr));                                                 \
    }
#define RF_C6_NOASM
#define RF_C6_COMMA_W , "+s"(wn8)
#define RF_C6_LOAD_WINDOW(IDX)                                                                   \
    {                                                                                            \
        const float *wp_ = swsym + (IDX);                                                        \
        asm volatile("s_load_dwordx8 %0, %1, 0x0" : "=&s"(wn8) : "s"(wp_));                      \
    }

    // One group of four steps: steps 0, 1 read columns 2, 3 through (ta, tb), steps 2, 3 read columns 0, 1 of
    // the next group - or of the next row's first one - through (TA2, TB2) at the offsets O2, O3; step 3
    // requests the window at index WIDX, which the group hands on by copy.  F0 B0 .. F3 B3: the front and back
    // masks of the steps.  First group of a row: backs [1, 3, 7, 15], the fronts of its columns 1..3 [3, 7, 15]
    // (column 0's came from the row before); last group: backs [15, 14, 12, 8], fronts [14, 12, 8] and [1] for
    // the next row's column 0; a row of one group: backs [1, 2, 4, 8], fronts [3, 4, 8] and [1].
#define RF_C6_GROUP(F, TA2, TB2, O2, O3, WIDX, F0, B0, F1, B1, F2, B2, F3, B3)                              \
    {                                                                                                       \
        float wv[8];                                                                                        \
        wv[0] = ws8[0]; wv[1] = ws8[1]; wv[2] = ws8[2]; wv[3] = ws8[3];                                     \
        wv[4] = ws8[4]; wv[5] = ws8[5]; wv[6] = ws8[6]; wv[7] = ws8[7];                                     \
        RF_C6_STEP(F, 0, gg[0], gg[1], ta, tb, 0, RF_C6_NOASM, , F0, B0)                                    \
        RF_C6_STEP(F, 1, gg[1], gg[0], ta, tb, Q4, RF_C6_NOASM, , F1, B1)                                   \
        RF_C6_STEP(F, 2, gg[0], gg[1], TA2, TB2, O2, RF_C6_NOASM, , F2, B2)                                 \
        RF_C6_STEP(F, 3, gg[1], gg[0], TA2, TB2, O3, RF_C6_LOAD_WINDOW(WIDX), RF_C6_COMMA_W, F3, B3)        \
        ws8 = wn8;                                                                                          \
    }
#define RF_C6_ROW_LOOP(F)                                                                         \
    for (int i = i_lo; i <= i_hi; i++) {                                                            \
        uint32_t ta_next, tb_next, ta2_next, tb2_next, wa_next;                                     \
        int ngroups_next;                                                                           \
        row_addr(i < i_hi ? i + 1 : i, ta_next, tb_next, ta2_next, tb2_next, wa_next,               \
                 ngroups_next);                                                                     \
        /* first group, full groups, last group; a row of one group (half-width 0) runs the single form    \
            instead.  Ifs without else, each but the first on a value the compiler cannot see through (see  \
            RF_L2_ROW_LOOP: an if / else around statements of the loop costs a copy of its registers). */   \
        int csel = ngroups < 2 ? ngroups : 2; /* 1: one group; 2: two or more */                            \
        if (csel == 2) {                                                                                    \
            wa_addr -= 4;                                                                                   \
            RF_C6_GROUP(F, ta2, tb2, 1, Q4 + 1, wa_addr, RF_L2_M3, RF_L2_M1, RF_L2_M7, RF_L2_M3,            \
                        RF_L2_M15, RF_L2_M7, RF_L2_M15, RF_L2_M15)                                          \
            ta += 4;                                                                                        \
            tb += 2;                                                                                        \
            ta2 += 4;                                                                                       \
            tb2 += 2;                                                                                       \
        }                                                                                                   \
        for (int gq = ngroups - 2; gq > 0; gq--) {                                                          \
            wa_addr -= 4;                                                                                   \
            RF_C6_GROUP(F, ta2, tb2, 1, Q4 + 1, wa_addr, RF_L2_M15, RF_L2_M15, RF_L2_M15, RF_L2_M15,        \
                        RF_L2_M15, RF_L2_M15, RF_L2_M15, RF_L2_M15)                                         \
            ta += 4;                                                                                        \
            tb += 2;                                                                                        \
            ta2 += 4;                                                                                       \
            tb2 += 2;                                                                                       \
        }                                                                                                   \
        /* the closing group reads ahead into the next row: the columns past the end of this row carry no   \
            weight, steps 2 and 3 read the next row's columns 0 and 1, step 3 forms its column 0 [1] */      \
        asm volatile("" : "+s"(csel));                                                                      \
        csel = __builtin_amdgcn_readfirstlane(csel);                                                        \
        if (csel == 2) {                                                                                    \
            RF_C6_GROUP(F, ta2_next, tb2_next, 0, Q4, wa_next, RF_L2_M14, RF_L2_M15, RF_L2_M12, RF_L2_M14,  \
                        RF_L2_M8, RF_L2_M12, RF_L2_M1, RF_L2_M8)                                            \
        }                                                                                                   \
        asm volatile("" : "+s"(csel));                                                                      \
        csel = __builtin_amdgcn_readfirstlane(csel);                                                        \
        if (csel == 1) {                                                                                    \
            RF_C6_GROUP(F, ta2_next, tb2_next, 0, Q4, wa_next, RF_L2_M3, RF_L2_M1, RF_L2_M4, RF_L2_M2,      \
                        RF_L2_M8, RF_L2_M4, RF_L2_M1, RF_L2_M8)                                             \
        }                                                                                                   \
        ta = ta_next;                                                                               \
        tb = tb_next;                                                                               \
        ta2 = ta2_next;                                                                             \
        tb2 = tb2_next;                                                                             \
        wa_addr = wa_next;                                                                          \
        ngroups = ngroups_next;                                                                     \
    }
    if constexpr (MSAD) {
        RF_C6_ROW_LOOP(MSAD)
    } else {
        RF_C6_ROW_LOOP(AND)
    }
#undef RF_C6_ROW_LOOP
#undef RF_C6_AND_AND
#undef RF_C6_AND_MSAD
#undef RF_C6_TJOUT_AND
#undef RF_C6_TJOUT_MSAD
#undef RF_C6_MASKIN_AND
#undef RF_C6_MASKIN_MSAD
#undef RF_C6_SAD_AND
#undef RF_C6_SAD_MSAD
#undef RF_C6_LOAD_WINDOW
#undef RF_C6_COMMA_W
#undef RF_C6_NOASM
#undef RF_C6_STEP
#undef RF_C6_GROUP
#undef RF_C6_CH
#undef RF_C6_CADD
#undef RF_C6_CMUL
#undef RF_C6_GATHER
#undef RF_C6_ADR
#undef RF_C6_WADD
#undef RF_C6_WMUL
}
// the live masks of the end groups, shared by jbf_tap_loop_grey4_la2 and jbf_tap_loop_rgb6
#undef RF_L2_STR
#undef RF_L2_STR_P
#undef RF_L2_ON
#undef RF_L2_ON_E
#undef RF_L2_ON_P
#undef RF_L2_ON_1
#undef RF_L2_ON_0
#undef RF_L2_SELK
#undef RF_L2_SEL3
#undef RF_L2_SEL2
#undef RF_L2_SEL1
#undef RF_L2_SEL0
#undef RF_L2_M0
#undef RF_L2_M1
#undef RF_L2_M2
#undef RF_L2_M3
#undef RF_L2_M4
#undef RF_L2_M7
#undef RF_L2_M8
#undef RF_L2_M12
#undef RF_L2_M14
#undef RF_L2_M15
#undef RF_LDS_READ_B64
#undef RF_LDS_READ_B128
#undef RF_LDS_READ_B32
#undef RF_LDS_READ_B32_OFF
#undef RF_LDS_READ_U16_OFF

}  // namespace
}  // namespace rf
