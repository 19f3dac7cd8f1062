// rf_augment_api.hip -- version and error text of librf_augment_hip.so.
#include "rf_augment_common.hpp"

namespace rfa {

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

}  // namespace rfa

extern "C" int rf_augment_version(void) { return RF_AUGMENT_VERSION; }

extern "C" const char *rf_augment_last_error(void) { return rfa::last_error_buf(); }
