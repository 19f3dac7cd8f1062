// rf_train_api.hip -- version and error text of librf_train_hip.so.
#include "rf_train_common.hpp"

namespace rft {

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

}  // namespace rft

extern "C" int rf_train_version(void) { return RF_TRAIN_VERSION; }

extern "C" const char *rf_train_last_error(void) { return rft::last_error_buf(); }
