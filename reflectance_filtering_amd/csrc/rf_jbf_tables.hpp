// rf_jbf_tables.hpp -- the joint bilateral's device parameter tables (rf_jbf_tables.hip) as their
// users see them: rf_jbf_u8 (rf_jbf.hip) and rf_jbf_f32 (rf_jbf_f32.hip).  Host only.
#pragma once
#include <memory>
#include <vector>

#include "rf_common.hpp"

namespace rf {

struct JbfTables {
    int device = -1;
    int radius = 0;
    int joint_cn = 0;
    double sigma_color = 0, sigma_space = 0;
    int maxk = 0;
    int lut_len = 0;   // entries kept: indices >= lut_len-1 are clamped (LUT value exactly 0)
    float *d_lut = nullptr;     // [256*joint_cn]
    int *d_di = nullptr;        // [maxk]
    int *d_dj = nullptr;        // [maxk]
    float *d_sw = nullptr;      // [maxk]
    int *d_hw = nullptr;        // [2r+1] half-width of the disk on tap row i
    // weight rows |i| = 0..r, each sw_len = 2*(r4+8) floats, centre at index r4+8, zeros outside
    // the disk (the weights are symmetric in i and in j)
    int r4 = 0, sw_len = 0;
    float *d_swsym = nullptr;
    std::shared_ptr<void> keep;  // JbfTableOwner of the arrays above
};

// The fields of a parameter set that need no device - radius, joint_cn, the sigmas, r4, sw_len and
// lut_len - which is all the launch plans read (rf_debug_jbf_ragged_plan); get_tables starts from it.
// lut: the colour table (jbf_colour_lut).
JbfTables jbf_host_tables(int radius, int joint_cn, double sigma_color, double sigma_space,
                          std::vector<float> &lut);

// While alive, this thread may make the "unsafe" runtime calls (allocation, creation of events,
// synchronisation of OTHER streams) although one of its streams is capturing: the first use of a
// parameter set inside a graph capture allocates its tables (hipStreamCaptureModeRelaxed for this
// thread only; the mode is put back on the way out).
struct CaptureRelax {
    hipStreamCaptureMode mode = hipStreamCaptureModeRelaxed;
    bool ok;
    CaptureRelax() { ok = hipThreadExchangeStreamCaptureMode(&mode) == hipSuccess; }
    ~CaptureRelax()
    {
        if (ok)
            (void)hipThreadExchangeStreamCaptureMode(&mode);
    }
};

// A call's reference to its tables: if it turns out to be the last one (the entry was evicted while
// the call was being enqueued), the arrays go to g_retired instead of being freed under the call.
struct TablesHold {
    JbfTables &t;
    ~TablesHold();
};

// The tables of one parameter set on the current device, from the cache or built and uploaded now.
int get_tables(int radius, int joint_cn, double sigma_color, double sigma_space, hipStream_t stream,
               JbfTables *out);

// rf_shutdown: empties the cache (arrays are freed by their owners).
void jbf_shutdown();

}  // namespace rf
