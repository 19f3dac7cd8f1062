// rf_jbf_common.hpp -- what the full-image joint bilateral (rf_jbf.hip) and its point form
// (rf_jbf_points.hip) share: the host code that builds the parameter tables and the per-pixel
// texel load and finish of jbf_generic_kernel.  One definition each, so the two entry points
// cannot drift apart.
#pragma once
#include <vector>

#include "rf_common.hpp"

namespace rf {

// Colour weights exp(i^2 * -0.5 / sigma_color^2) rounded to float, i = 0 .. 256*joint_cn - 1,
// computed in double with libm's exp like jointBilateralFilter_8u.  Returns the number of entries
// up to and including the first exact zero (the table is non-increasing: every later entry is 0).
int jbf_colour_lut(int joint_cn, double sigma_color, std::vector<float> &lut);

// The taps of the radius-r disk in OpenCV's row-major order: offsets (di, dj), spatial weights
// exp(r^2 * -0.5 / sigma_space^2) rounded to float, and hw[i + r] = the disk's half-width on row i.
void jbf_space_taps(int radius, double sigma_space, std::vector<int> &di, std::vector<int> &dj,
                    std::vector<float> &sw, std::vector<int> &hw);

// Packs up to 3 interleaved bytes into the low bytes of a dword (byte 3 = 0), so that
// v_sad_u8 on two such dwords is the L1 colour distance.
// cn = -1: single-channel image treated as three equal channels (RF_JBF_GREY_AS_BGR).
__device__ inline uint32_t load_packed(const uint8_t *img, size_t pix, int cn)
{
    if (cn < 0)
        return (uint32_t)img[pix] * 0x010101u;
    const uint8_t *p = img + pix * cn;
    uint32_t v = p[0];
    if (cn == 3)
        v |= ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16);
    return v;
}

// dst bytes of one pixel from its sums: sum * (1/wsum), or sum / wsum under RF_JBF_TRUE_DIVISION,
// saturated like saturate_cast<uchar>.
__device__ inline void finish_pixel(uint8_t *o, const float *sum, float wsum, int scn, int flags)
{
    if (flags & RF_JBF_TRUE_DIVISION) {
        for (int c = 0; c < scn; c++)
            o[c] = saturate_u8(__fdiv_rn(sum[c], wsum));
    } else {
        const float inv = __fdiv_rn(1.0f, wsum);
        for (int c = 0; c < scn; c++)
            o[c] = saturate_u8(__fmul_rn(sum[c], inv));
    }
}

}  // namespace rf
