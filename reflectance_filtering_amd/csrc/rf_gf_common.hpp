// rf_gf_common.hpp -- what the guided-filter units (rf_gf.hip, rf_gf_f32.hip, rf_gf_side.hip) share:
// the argument rules of the entry points, the launch rule for a chunk of images and the side-stream
// table.  One definition each, so the entry points cannot drift apart.
#pragma once
#include "rf_common.hpp"

namespace rf {

// ---- argument rules -----------------------------------------------------------------------
// Each returns RF_OK or the fail(...) it produced; `who` names the entry in the message.  An entry
// calls them in its own order (the order decides which of two broken rules a caller hears about).
constexpr int kGfMaxRadius = 4096;  // a larger radius is refused

// the flag bits a caller may pass
inline int gf_check_flags(const char *who, int flags)
{
    if (flags & ~RF_GF_GREY_AS_BGR)
        return fail(RF_E_BADARG, "%s: unknown flag bits 0x%x", who, (unsigned)(flags & ~RF_GF_GREY_AS_BGR));
    return RF_OK;
}

// a grey guide (RF_GF_GREY_AS_BGR) is one byte per pixel that stands for three equal channels; any
// other guide has three
inline int gf_check_guide(const char *who, int guide_cn, bool grey)
{
    if (grey && guide_cn == 3)
        return fail(RF_E_BADARG, "%s: RF_GF_GREY_AS_BGR takes a 1-channel guide (got 3 channels)", who);
    if (grey && guide_cn != 1)
        return fail(RF_E_UNSUPPORTED, "%s: RF_GF_GREY_AS_BGR takes a 1-channel guide (got %d)", who,
                    guide_cn);
    if (!grey && guide_cn != 3)
        return fail(RF_E_UNSUPPORTED, "%s: guide must have 3 channels (got %d)", who, guide_cn);
    return RF_OK;
}

inline int gf_check_src_cn(const char *who, int src_cn)
{
    if (src_cn != 1 && src_cn != 3)
        return fail(RF_E_UNSUPPORTED, "%s: src channels must be 1 or 3 (got %d)", who, src_cn);
    return RF_OK;
}

inline int gf_check_radius(const char *who, int radius)
{
    if (radius < 0 || radius > kGfMaxRadius)
        return fail(RF_E_UNSUPPORTED, "%s: radius %d outside 0..4096", who, radius);
    return RF_OK;
}

// the 8-bit kernels address a row's alpha/beta (16 B per pixel) with 32-bit offsets.  image >= 0: the
// width is that of image `image` of a list
inline int gf_check_width(const char *who, int w, int image = -1)
{
    if (w < (1 << 27))
        return RF_OK;
    if (image >= 0)
        return fail(RF_E_UNSUPPORTED, "%s: width %d of image %d beyond 2^27 - 1", who, w, image);
    return fail(RF_E_UNSUPPORTED, "%s: width %d beyond 2^27 - 1", who, w);
}

// experiments without a grey-guide form (reflectance_filtering_debug.h)
inline int gf_check_grey_debug(const char *who, bool grey)
{
    if (grey && (debug_get(kDbgGfGuideCache) || debug_get(kDbgGfExact)))
        return fail(RF_E_UNSUPPORTED, "%s: RF_GF_GREY_AS_BGR has no form for the debug options "
                    "gf_guide_cache / gf_exact", who);
    return RF_OK;
}

// dst may equal src but overlap neither it partially nor the guide.  px pixels of guide_cn / src_cn
// elements of `elem` bytes each
inline int gf_check_overlap(const char *who, const void *guide, const void *src, const void *dst,
                            size_t px, int guide_cn, int src_cn, size_t elem)
{
    const size_t dst_bytes = px * src_cn * elem;
    if (ranges_overlap(dst, dst_bytes, guide, px * guide_cn * elem))
        return fail(RF_E_BADARG, "%s: dst must not overlap guide", who);
    if (dst != src && ranges_overlap(dst, dst_bytes, src, dst_bytes))
        return fail(RF_E_BADARG, "%s: dst may equal src but not partially overlap it", who);
    return RF_OK;
}

// ---- the launch rule for a chunk of the uniform entries (rf_gf.hip) --------------------------
bool gf_chunk_fits(int m, int h, int w, int src_cn, bool float_kernels);
int gf_launch_chunk(int chunk, int h, int w, int src_cn, bool float_kernels);

// ---- side streams (rf_gf_side.hip) -----------------------------------------------------------
// The library's side stream for `caller` (nullptr: none to be had - run on the caller's stream alone),
// held until gf_side_release; gf_shutdown destroys them all.
hipStream_t gf_side_stream(hipStream_t caller);
void gf_side_release(hipStream_t side);
void gf_shutdown();

}  // namespace rf
