// rf_jbf_common.hpp -- what the full-image joint bilateral (rf_jbf.hip, rf_jbf_f32.hip) and its
// point form (rf_jbf_points.hip) share: the argument rules of the entry points, the host code that
// builds the parameter tables (defined in rf_jbf_tables.hip) and the per-pixel texel load and finish
// of jbf_generic_kernel.  One definition each, so the entry points cannot drift apart.
#pragma once
#include <cmath>
#include <vector>

#include "rf_common.hpp"

namespace rf {

// ---- argument rules (OpenCV's, and the library's limits) ----------------------------------
// the flag bits a caller may pass
constexpr int kJbfPublicFlags = RF_JBF_TRUE_DIVISION | RF_JBF_FORCE_GENERIC | RF_JBF_GREY_AS_BGR;
constexpr int kJbfMaxRadius = 4096;  // a larger radius is refused

// non-positive sigmas become 1
inline double jbf_sigma(double sigma) { return sigma <= 0 ? 1 : sigma; }

// radius from d, or from sigma_space (after jbf_sigma) when d <= 0; at least 1
inline int jbf_radius(int d, double sigma_space)
{
    const int radius = d <= 0 ? (int)std::lrint(sigma_space * 1.5) : d / 2;
    return radius < 1 ? 1 : radius;
}

// RF_JBF_GREY_AS_BGR affects a 1-channel joint only: it counts as 3 equal channels (colour
// distance 3*|d|, 766-entry LUT), so the tables are those of 3 channels ...
inline int jbf_table_cn(int joint_cn, int flags)
{
    return joint_cn == 1 && (flags & RF_JBF_GREY_AS_BGR) ? 3 : joint_cn;
}
// ... and the kernels get joint_cn = -1 and replicate the byte (load_packed)
inline int jbf_kernel_cn(int joint_cn, int flags)
{
    return joint_cn == 1 && (flags & RF_JBF_GREY_AS_BGR) ? -1 : joint_cn;
}

// channel counts and border type every u8 entry accepts; `who` names the entry in the message
inline int jbf_check_format(const char *who, int joint_cn, int src_cn, int border)
{
    if ((joint_cn != 1 && joint_cn != 3) || (src_cn != 1 && src_cn != 3))
        return fail(RF_E_UNSUPPORTED, "%s: channels must be 1 or 3 (joint %d, src %d)", who,
                    joint_cn, src_cn);
    if (border < 0 || border > 4)
        return fail(RF_E_UNSUPPORTED, "%s: border type %d", who, border);
    return RF_OK;
}

// The grey map of rf_jbf_u8's two-workgroups-per-CU route (rf_jbf_greymap.hip): the route's byte per 64x64
// tile from one pass over the images.  jbf_grey_map_serves: may a call take it (else every tile scans its
// region); jbf_launch_grey_map: the launch that sets the bytes to "grey" and the pass, on `stream`.
bool jbf_grey_map_serves(int h, int w, int radius, int border, int tiles_x, int tiles_y);
int jbf_launch_grey_map(const uint8_t *joint, const uint8_t *src, int n, int h, int w, int jcn, int scn,
                        int radius, int border, hipStream_t stream, int tiles_x, int tiles_y,
                        uint8_t *tile_flags);

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
