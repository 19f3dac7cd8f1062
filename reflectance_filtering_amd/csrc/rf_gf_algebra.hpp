// rf_gf_algebra.hpp -- the guided filter's quantities and its per-pixel algebra: what the 8-bit stage 1
// (rf_gf_stage1.hpp) and the float kernels (rf_gf_f32.hip) share.  Quant names the order of the box-summed
// quantities, gf_pixel_algebra turns their window means into alpha/beta with the separately rounded float
// operations of guided_filter.cpp.  One definition, so the two paths cannot drift apart.
#pragma once
#include "rf_gf_fused.hpp"

namespace rf {
namespace {

// Stage-1 quantities.  GUIDE = true: all of them, q: 0..2 I_g | 3..8 I_aI_b (00 01 02 11 12 22) |
// 9.. p_s | then p_s*I_g (s major).  GUIDE = false (later passes of an iterated call, whose guide
// statistics come from the record the first pass left): only p_s | p_s*I_g.
template <int SCN, bool GUIDE = true>
struct Quant {
    static constexpr int G0 = GUIDE ? 9 : 0;  // first src quantity
    static constexpr int NQ = G0 + 4 * SCN;
    // acc[q] += (NEG ? -1 : +1) * quantity q of the pixel with guide bytes g0..g2 and src bytes p[]
    // (uint32 wrap-around is exact).  A row that leaves the window is added with one factor of
    // every product negated: one v_mad_i32_i24 per product either way, instead of a multiply and
    // a subtract.
    template <bool NEG>
    __device__ static inline void accumulate(int g0, int g1, int g2, const int *p, uint32_t *acc)
    {
        const int s0 = NEG ? -g0 : g0, s1 = NEG ? -g1 : g1, s2 = NEG ? -g2 : g2;
        if (GUIDE) {
            acc[0] += (uint32_t)s0;
            acc[1] += (uint32_t)s1;
            acc[2] += (uint32_t)s2;
            acc[3] += (uint32_t)(s0 * g0);
            acc[4] += (uint32_t)(s0 * g1);
            acc[5] += (uint32_t)(s0 * g2);
            acc[6] += (uint32_t)(s1 * g1);
            acc[7] += (uint32_t)(s1 * g2);
            acc[8] += (uint32_t)(s2 * g2);
        }
#pragma unroll
        for (int s = 0; s < SCN; s++) {
            const int ps = NEG ? -p[s] : p[s];
            acc[G0 + s] += (uint32_t)ps;
            acc[G0 + SCN + 3 * s + 0] += (uint32_t)(ps * g0);
            acc[G0 + SCN + 3 * s + 1] += (uint32_t)(ps * g1);
            acc[G0 + SCN + 3 * s + 2] += (uint32_t)(ps * g2);
        }
    }
};

// index into the 6-entry symmetric store: (0,0)=0 (0,1)=1 (0,2)=2 (1,1)=3 (1,2)=4 (2,2)=5
__device__ constexpr int sym(int i, int j)
{
    return i <= j ? (i * 3 - i * (i - 1) / 2 + (j - i)) : (j * 3 - j * (j - 1) / 2 + (i - j));
}

// Per-pixel algebra of guided_filter.cpp, every operation the separately rounded float op of the
// corresponding OpenCV helper, in two halves:
//   gf_guide_algebra  from the 9 guide means m (order of Quant): covariance of the guide (+eps on
//                     the diagonal) and its inverse by cofactors -> gs[0..2] = mean I_g,
//                     gs[3..8] = inverse (symmetric store).  Depends on the guide only: the passes
//                     of an iterated call share it (kGsFloats floats per pixel).
//   gf_src_algebra    from gs and the 4*SCN src means ms (p_s | p_s*I_g): for every src channel s
//                     the coefficients alpha_{s,g} (out[4s + g]) and beta_s (out[4s + 3]).
constexpr int kGsFloats = kGsFloatsPublic;

// out[i] = num[i] / den for six numerators, every quotient the correctly rounded IEEE result
// (__fdiv_rn), i.e. what OpenCV's per-element division gives.  hipcc expands an IEEE division into
// v_div_scale x 2, v_rcp, two FMAs that refine the reciprocal, a multiply, three FMAs, v_div_fmas
// and v_div_fixup (46 issue cycles); the reciprocal and its refinement depend on the denominator
// alone as long as v_div_scale leaves both operands unscaled, which it does whenever the
// exponents are far from the float range's ends.  That case is recognised up front (|den| in
// [2^-30, 2^50], every numerator zero or in [2^-40, 2^36]: no scaling, no denormal quotient) and
// runs the SAME instruction sequence with the denominator's part done once; v_div_fixup stays,
// it is what gives a zero numerator its sign.  Anything else takes the plain divisions.
__device__ inline void div6_by(const float *num, float den, float *out)
{
    // |den| in [2^-30, 2^50]; every numerator zero or in [2^-40, 2^36].  The upper bound is tested on
    // the SUM of the magnitudes (source modifiers, no masking instructions; a NaN or an infinity
    // anywhere propagates and fails the comparison; a sum above 2^36 whose terms are all below it
    // merely takes the plain divisions); the smallest non-zero numerator is an unsigned minimum
    // over (bits << 1) - 2, which drops the sign and sends a zero to the top (one v_lshl_add_u32
    // per numerator).
    const float ad = fabsf(den);
    const float hi = ((fabsf(num[0]) + fabsf(num[1])) + (fabsf(num[2]) + fabsf(num[3]))) +
                     (fabsf(num[4]) + fabsf(num[5]));
    uint32_t lo = 0xffffffffu;
#pragma unroll
    for (int i = 0; i < 6; i++)
        lo = min(lo, (__float_as_uint(num[i]) << 1) - 2u);
    // (comparisons written so that a NaN anywhere fails them)
    const bool fast = ad >= 0x1p-30f && ad <= 0x1p50f && hi <= 0x1p36f &&
                      lo >= (0x2b800000u << 1) - 2u;  // 2^-40
    if (fast) {
        const float r0 = __builtin_amdgcn_rcpf(den);
        const float e = __fmaf_rn(-den, r0, 1.0f);
        const float r1 = __fmaf_rn(e, r0, r0);
#pragma unroll
        for (int i = 0; i < 6; i++) {
            const float q0 = __fmul_rn(num[i], r1);
            const float t = __fmaf_rn(-den, q0, num[i]);
            const float q1 = __fmaf_rn(t, r1, q0);
            const float t2 = __fmaf_rn(-den, q1, num[i]);
            out[i] = __builtin_amdgcn_div_fixupf(__fmaf_rn(t2, r1, q1), den, num[i]);
        }
    } else {
#pragma unroll
        for (int i = 0; i < 6; i++)
            out[i] = __fdiv_rn(num[i], den);
    }
}

__device__ inline void gf_guide_algebra(const float *m, float eps_f, int eps_small, float *gs)
{
    const float *mI = m;
    float cov[6];
    // cov(c1,c2) = mean(I1*I2) - mean1*mean2 ; diagonal: - (mean*mean + (-eps))
    cov[sym(0, 1)] = __fsub_rn(m[4], __fmul_rn(mI[0], mI[1]));
    cov[sym(0, 2)] = __fsub_rn(m[5], __fmul_rn(mI[0], mI[2]));
    cov[sym(1, 2)] = __fsub_rn(m[7], __fmul_rn(mI[1], mI[2]));
    cov[sym(0, 0)] = __fsub_rn(m[3], __fadd_rn(__fmul_rn(mI[0], mI[0]), -eps_f));
    cov[sym(1, 1)] = __fsub_rn(m[6], __fadd_rn(__fmul_rn(mI[1], mI[1]), -eps_f));
    cov[sym(2, 2)] = __fsub_rn(m[8], __fadd_rn(__fmul_rn(mI[2], mI[2]), -eps_f));
    float inv[6];
#pragma unroll
    for (int kk = 0; kk < 3; kk++)
#pragma unroll
        for (int l = 0; l <= kk; l++) {
            const float a00 = cov[sym((kk + 1) % 3, (l + 1) % 3)];
            const float a01 = cov[sym((kk + 1) % 3, (l + 2) % 3)];
            const float a10 = cov[sym((kk + 2) % 3, (l + 1) % 3)];
            const float a11 = cov[sym((kk + 2) % 3, (l + 2) % 3)];
            inv[sym(kk, l)] = __fsub_rn(__fmul_rn(a00, a11), __fmul_rn(a01, a10));
        }
    float det = __fmul_rn(cov[sym(0, 0)], inv[sym(0, 0)]);
    det = __fadd_rn(det, __fmul_rn(cov[sym(1, 0)], inv[sym(1, 0)]));
    det = __fadd_rn(det, __fmul_rn(cov[sym(2, 0)], inv[sym(2, 0)]));
    if (eps_small && fabsf(det) < 1e-6f)
        det = 1.f;
    gs[0] = mI[0];
    gs[1] = mI[1];
    gs[2] = mI[2];
    div6_by(inv, det, gs + 3);
}

template <int SCN>
__device__ inline void gf_src_algebra(const float *gs, const float *ms, float *out)
{
    const float *mI = gs, *inv = gs + 3;
#pragma unroll
    for (int s = 0; s < SCN; s++) {
        const float mp = ms[s];
        float cp[3];
#pragma unroll
        for (int g = 0; g < 3; g++)
            cp[g] = __fsub_rn(ms[SCN + 3 * s + g], __fmul_rn(mp, mI[g]));
        float beta = mp;
#pragma unroll
        for (int g = 0; g < 3; g++) {
            float a = __fmul_rn(inv[sym(g, 0)], cp[0]);
            a = __fadd_rn(a, __fmul_rn(inv[sym(g, 1)], cp[1]));
            a = __fadd_rn(a, __fmul_rn(inv[sym(g, 2)], cp[2]));
            out[4 * s + g] = a;
            beta = __fsub_rn(beta, __fmul_rn(a, mI[g]));
        }
        out[4 * s + 3] = beta;
    }
}

// both halves: from the 9 + 4*SCN window means m (order of Quant<SCN, true>)
template <int SCN>
__device__ inline void gf_pixel_algebra(const float *m, float eps_f, int eps_small, float *out)
{
    float gs[kGsFloats];
    gf_guide_algebra(m, eps_f, eps_small, gs);
    gf_src_algebra<SCN>(gs, m + 9, out);
}

}  // namespace
}  // namespace rf
