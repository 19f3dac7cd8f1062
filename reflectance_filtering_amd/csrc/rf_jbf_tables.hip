// rf_jbf_tables.hip -- parameter tables of the joint bilateral filter (colour LUT, tap tables) and
// their cache: one device arena per parameter set, uploaded once when the set is first seen
// (get_tables); entries a captured graph points into are pinned.  The host functions that compute
// the tables (jbf_colour_lut, jbf_space_taps; rf_jbf_common.hpp) are shared with the point form.
#include <atomic>
#include <cmath>
#include <cstring>
#include <mutex>
#include <vector>

#include "rf_jbf_common.hpp"
#include "rf_jbf_tables.hpp"

namespace rf {

int jbf_colour_lut(int joint_cn, double sigma_color, std::vector<float> &lut)
{
    const double gauss_color_coeff = -0.5 / (sigma_color * sigma_color);
    const int nlut = 256 * joint_cn;
    lut.assign(nlut, 0.0f);
    for (int i = 0; i < nlut; i++)
        lut[i] = (float)std::exp(i * i * gauss_color_coeff);
    for (int i = 0; i < nlut; i++)
        if (lut[i] == 0.0f)
            return i + 1;
    return nlut;
}

void jbf_space_taps(int radius, double sigma_space, std::vector<int> &di, std::vector<int> &dj,
                    std::vector<float> &sw, std::vector<int> &hw)
{
    const double gauss_space_coeff = -0.5 / (sigma_space * sigma_space);
    di.clear();
    dj.clear();
    sw.clear();
    hw.assign(2 * radius + 1, -1);
    for (int i = -radius; i <= radius; i++)
        for (int j = -radius; j <= radius; j++) {
            double r = std::sqrt((double)i * i + (double)j * j);
            if (r > radius)
                continue;
            float wgt = (float)std::exp(r * r * gauss_space_coeff);
            di.push_back(i);
            dj.push_back(j);
            sw.push_back(wgt);
            if (j >= 0 && j > hw[i + radius])
                hw[i + radius] = j;
        }
}

namespace {

// Owns the arrays of one cache entry: ONE device arena, uploaded once when the entry is built - on a
// stream of its own, waited for there, before the entry is published (the one host wait of a
// parameter set's first use, tens of microseconds; every later call only enqueues kernels).  The
// caller's stream may be capturing meanwhile: nothing of the upload enters its graph.
// rf_jbf_u8 keeps a reference for the duration of the call, so an eviction (or rf_shutdown) on
// another thread cannot free tables that a call has looked up but not launched yet; the last
// reference frees them on their own device (hipFree waits for the work queued there).  A graph that
// captured a call bakes in pointers into the arena: an entry that was ever looked up on a capturing
// stream is PINNED - never evicted, freed by rf_shutdown only (destroy such graphs
// before rf_shutdown).
struct JbfTableOwner {
    int device = 0;
    void *d_arena = nullptr;
    size_t bytes = 0;
    std::atomic<bool> pinned{false};  // referenced by a captured graph
    ~JbfTableOwner()
    {
        int cur = 0;
        const bool switched = hipGetDevice(&cur) == hipSuccess && cur != device &&
                              hipSetDevice(device) == hipSuccess;
        if (d_arena)
            (void)hipFree(d_arena);
        if (switched)
            (void)hipSetDevice(cur);
    }
};

std::mutex g_mu;
std::vector<JbfTables> g_tables;
// Owners that left the cache (evicted entries, entries a finishing call held the last reference
// to): their arrays are freed by the next call that builds a set of tables on a stream that is NOT
// capturing - hipFree inside a capture invalidates it, and it waits for the whole device, which a call
// that finds its tables cached must not do - or by rf_shutdown.
std::vector<std::shared_ptr<void>> g_retired;

void drain_retired(hipStream_t stream)
{
    if (stream_is_capturing(stream))
        return;
    std::vector<std::shared_ptr<void>> bin;
    {
        std::lock_guard<std::mutex> lock(g_mu);
        bin.swap(g_retired);
    }
    if (!bin.empty()) {
        CaptureRelax relax;  // (another thread of the process may be capturing in the global mode)
        bin.clear();
    }
}

// The entry is about to be used by work enqueued on `stream`: if that stream is capturing, the graph
// will hold pointers into the entry's arena for as long as it lives - pin the entry.
void note_use_on(const JbfTables &t, hipStream_t stream)
{
    if (stream_is_capturing(stream))
        static_cast<JbfTableOwner *>(t.keep.get())->pinned.store(true, std::memory_order_relaxed);
}

}  // namespace

TablesHold::~TablesHold()
{
    if (t.keep && t.keep.use_count() == 1) {
        std::lock_guard<std::mutex> lock(g_mu);
        g_retired.push_back(std::move(t.keep));
    }
}

JbfTables jbf_host_tables(int radius, int joint_cn, double sigma_color, double sigma_space,
                          std::vector<float> &lut)
{
    JbfTables t;
    t.radius = radius;
    t.joint_cn = joint_cn;
    t.sigma_color = sigma_color;
    t.sigma_space = sigma_space;
    // keep entries up to and including the first exact zero (the LUT is non-increasing)
    t.lut_len = jbf_colour_lut(joint_cn, sigma_color, lut);
    t.r4 = (radius + 3) & ~3;
    t.sw_len = 2 * (t.r4 + 8);
    return t;
}

// Host-side parameter tables, computed in double exactly like jointBilateralFilter_8u does.
int get_tables(int radius, int joint_cn, double sigma_color, double sigma_space, hipStream_t stream,
               JbfTables *out)
{
    int dev = 0;
    RF_HIP_CHECK(hipGetDevice(&dev));
    {
        std::lock_guard<std::mutex> lock(g_mu);
        for (const JbfTables &t : g_tables)
            if (t.device == dev && t.radius == radius && t.joint_cn == joint_cn &&
                t.sigma_color == sigma_color && t.sigma_space == sigma_space) {
                *out = t;
                break;
            }
    }
    if (out->keep) {
        note_use_on(*out, stream);
        return RF_OK;
    }
    // Tables that left the cache are freed here, where a new set is built and the host waits anyway:
    // hipFree waits for the whole device, and a call that finds its tables cached must not (the header's
    // stream rules; tests/test_gpu_stream_contract.py).  A build evicts at most one entry, so the bin
    // stays small.
    drain_retired(stream);
    std::vector<float> lut;
    JbfTables t = jbf_host_tables(radius, joint_cn, sigma_color, sigma_space, lut);
    t.device = dev;
    const int nlut = 256 * joint_cn;
    const int d = 2 * radius + 1;
    std::vector<int> di, dj, hw;
    std::vector<float> sw;
    jbf_space_taps(radius, sigma_space, di, dj, sw, hw);
    t.maxk = (int)di.size();
    std::vector<float> swsym((size_t)(radius + 1) * t.sw_len, 0.0f);
    for (size_t k = 0; k < di.size(); k++)
        if (di[k] >= 0)
            swsym[(size_t)di[k] * t.sw_len + (t.r4 + 8) + dj[k]] = sw[k];
    // one arena: [swsym][lut][di][dj][sw][hw], every part 256-byte aligned
    const size_t part[6] = {sizeof(float) * swsym.size(), sizeof(float) * (size_t)nlut,
                            sizeof(int) * (size_t)t.maxk, sizeof(int) * (size_t)t.maxk,
                            sizeof(float) * (size_t)t.maxk, sizeof(int) * (size_t)d};
    const void *from[6] = {swsym.data(), lut.data(), di.data(), dj.data(), sw.data(), hw.data()};
    size_t off[6], total = 0;
    for (int k = 0; k < 6; k++) {
        off[k] = total;
        total += (part[k] + 255) & ~(size_t)255;
    }
    auto owner = std::make_shared<JbfTableOwner>();
    owner->device = dev;
    owner->bytes = total;
    t.keep = owner;
    {
        // allocation, upload on a private stream and the wait for it: "unsafe" calls while the
        // caller's stream may be capturing - admitted for this thread by CaptureRelax; the tables
        // are resident before anybody can find the entry
        std::vector<char> image(total, 0);
        for (int k = 0; k < 6; k++)
            std::memcpy(image.data() + off[k], from[k], part[k]);
        CaptureRelax relax;
        hipStream_t ps = nullptr;
        RF_HIP_CHECK(hipStreamCreateWithFlags(&ps, hipStreamNonBlocking));
        struct StreamGuard {
            hipStream_t s;
            ~StreamGuard() { (void)hipStreamDestroy(s); }
        } guard{ps};
        RF_HIP_CHECK(hipMalloc(&owner->d_arena, total));
        RF_HIP_CHECK(hipMemcpyAsync(owner->d_arena, image.data(), total, hipMemcpyHostToDevice, ps));
        RF_HIP_CHECK(hipStreamSynchronize(ps));
    }
    char *db = static_cast<char *>(owner->d_arena);
    t.d_swsym = reinterpret_cast<float *>(db + off[0]);
    t.d_lut = reinterpret_cast<float *>(db + off[1]);
    t.d_di = reinterpret_cast<int *>(db + off[2]);
    t.d_dj = reinterpret_cast<int *>(db + off[3]);
    t.d_sw = reinterpret_cast<float *>(db + off[4]);
    t.d_hw = reinterpret_cast<int *>(db + off[5]);
    {
        std::lock_guard<std::mutex> lock(g_mu);
        // (another thread may have built the same entry meanwhile: use that one, ours is freed)
        bool found = false;
        for (const JbfTables &e : g_tables)
            if (e.device == dev && e.radius == radius && e.joint_cn == joint_cn &&
                e.sigma_color == sigma_color && e.sigma_space == sigma_space) {
                g_retired.push_back(std::move(t.keep));  // ours: freed later, outside any capture
                t = e;
                found = true;
                break;
            }
        if (!found) {
            // bounded cache (parameter sweeps must not accumulate device memory): drop the oldest
            // entry that no captured graph refers to, of this device if there is one; its arrays are
            // freed when the last call using them returns.  Pinned entries stay: a cache of nothing
            // but pinned entries grows.
            if (g_tables.size() >= 64) {
                size_t victim = g_tables.size();
                for (size_t i = 0; i < g_tables.size(); i++) {
                    if (static_cast<JbfTableOwner *>(g_tables[i].keep.get())->pinned.load(
                            std::memory_order_relaxed))
                        continue;
                    if (victim == g_tables.size())
                        victim = i;
                    if (g_tables[i].device == dev) {
                        victim = i;
                        break;
                    }
                }
                if (victim != g_tables.size()) {
                    g_retired.push_back(std::move(g_tables[victim].keep));
                    g_tables.erase(g_tables.begin() + victim);
                }
            }
            g_tables.push_back(t);
        }
    }
    *out = t;
    note_use_on(*out, stream);
    return RF_OK;
}

void jbf_shutdown()
{
    std::lock_guard<std::mutex> lock(g_mu);
    g_tables.clear();  // arrays are freed by their owners (calls in flight keep theirs alive)
    g_retired.clear();
}

}  // namespace rf
