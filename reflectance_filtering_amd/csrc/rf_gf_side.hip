// rf_gf_side.hip -- the guided filter's side streams (host code only; declared in rf_gf_common.hpp).
#include <mutex>

#include "rf_gf_common.hpp"

namespace rf {

// Side streams for the second half of a batch, one per CALLER stream (so two callers never meet
// on one side stream, and a caller that captures its stream into a graph pulls only its own side
// stream into that capture).  The table is bounded: when it is full the least recently used entry
// whose side stream is idle is destroyed and replaced; if none is idle, or the caller's stream
// belongs to another device than the current one, the call runs on the caller's stream alone
// (nullptr).  An entry is held (busy) from gf_side_stream until the call that got it has enqueued
// everything (gf_side_release): an idle-looking stream is not taken from under a call that is
// about to use it.  rf_shutdown() destroys them all.
namespace {
struct SideStream {
    hipStream_t caller, side;
    int device;
    unsigned long long used;
    int busy;  // calls that hold this entry and may not have enqueued their work yet: never recycled
};
constexpr size_t kMaxSideStreams = 16;
std::mutex g_side_mu;
SideStream g_side[kMaxSideStreams];
size_t g_side_n = 0;
unsigned long long g_side_tick = 0;
}  // namespace

hipStream_t gf_side_stream(hipStream_t caller)
{
    int dev = 0, sdev = 0;
    if (hipGetDevice(&dev) != hipSuccess)
        return nullptr;
    if (caller != nullptr) {
        if (hipStreamGetDevice(caller, &sdev) != hipSuccess) {
            (void)hipGetLastError();
            return nullptr;
        }
        if (sdev != dev)
            return nullptr;
    }
    std::lock_guard<std::mutex> lock(g_side_mu);
    for (size_t i = 0; i < g_side_n; i++)
        if (g_side[i].caller == caller && g_side[i].device == dev) {
            g_side[i].used = ++g_side_tick;
            g_side[i].busy++;
            return g_side[i].side;
        }
    size_t slot = g_side_n;
    if (g_side_n == kMaxSideStreams) {
        slot = kMaxSideStreams;
        for (size_t i = 0; i < g_side_n; i++) {
            if (g_side[i].busy > 0 || (slot != kMaxSideStreams && g_side[i].used > g_side[slot].used))
                continue;
            hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
            if (hipStreamIsCapturing(g_side[i].side, &cap) != hipSuccess ||
                cap != hipStreamCaptureStatusNone || hipStreamQuery(g_side[i].side) != hipSuccess) {
                (void)hipGetLastError();
                continue;
            }
            slot = i;
        }
        if (slot == kMaxSideStreams)
            return nullptr;
        (void)hipStreamDestroy(g_side[slot].side);
    }
    hipStream_t st = nullptr;
    if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) {
        (void)hipGetLastError();
        if (slot != g_side_n) {  // the recycled entry is gone: close the gap
            g_side[slot] = g_side[g_side_n - 1];
            g_side_n--;
        }
        return nullptr;
    }
    g_side[slot] = {caller, st, dev, ++g_side_tick, 1};
    if (slot == g_side_n)
        g_side_n++;
    return st;
}

void gf_side_release(hipStream_t side)
{
    if (side == nullptr)
        return;
    std::lock_guard<std::mutex> lock(g_side_mu);
    for (size_t i = 0; i < g_side_n; i++)
        if (g_side[i].side == side && g_side[i].busy > 0) {
            g_side[i].busy--;
            return;
        }
}

void gf_shutdown()
{
    std::lock_guard<std::mutex> lock(g_side_mu);
    for (size_t i = 0; i < g_side_n; i++)
        (void)hipStreamDestroy(g_side[i].side);
    g_side_n = 0;
}

}  // namespace rf
