// rf_recover_api.hip -- version, error text and the shared argument rules of librf_recover_hip.so.
#include "rf_recover_common.hpp"

namespace rfr {

char *last_error_buf()
{
    static thread_local char buf[512] = "";
    return buf;
}

int fail(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(last_error_buf(), 512, fmt, ap);
    va_end(ap);
    return code;
}

int check_sizes(const char *who, long long npixels, long long nlisted)
{
    if (npixels < 0 || nlisted < 0)
        return fail(kBadArg, "%s: bad size P=%lld K=%lld", who, npixels, nlisted);
    if (npixels > 0x7fffffffll || nlisted > 0x7fffffffll)
        return fail(kUnsupported, "%s: too many pixels for one launch", who);
    return kOk;
}

int check_norm(const char *who, int norm)
{
    if (norm < RF_RECOVER_NORM_MEAN || norm > RF_RECOVER_NORM_NORM)
        return fail(kBadArg, "%s: unknown norm %d (0 Mean, 1 Max, 2 Y, 3 Norm)", who, norm);
    return kOk;
}

}  // namespace rfr

extern "C" int rf_recover_version(void) { return RF_RECOVER_VERSION; }

extern "C" const char *rf_recover_last_error(void) { return rfr::last_error_buf(); }
