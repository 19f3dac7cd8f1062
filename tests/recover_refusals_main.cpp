// drives the host-side refusals of librf_recover_hip.so's entries; built with the library's sources under
// -fsanitize=address,undefined (host code only).  Every call here returns before any device work.
#include <cmath>
#include <cstdio>
#include <cstring>

#include "reflectance_filtering_recover.h"

static int failures = 0;
#define EXPECT(call, code, text)                                                              \
    do {                                                                                      \
        int rc_ = (call);                                                                     \
        if (rc_ != (code) || !strstr(rf_recover_last_error(), text)) {                        \
            printf("line %d: %s -> %d '%s'\n", __LINE__, #call, rc_, rf_recover_last_error()); \
            failures++;                                                                       \
        }                                                                                     \
    } while (0)

int main()
{
    float *f = (float *)0x1000;
    double *d = (double *)0x1000;
    long long *q = (long long *)0x1000;
    void *ws = (void *)0x1000;
    const float nan = std::nanf(""), inf = INFINITY;
    size_t need = rf_recover_boundary_workspace_bytes(1000);
    int plan[3];
    EXPECT(rf_recover_version(), 100, "");
    EXPECT(rf_recover_forward_f32(nullptr, nullptr, 0, nullptr, 5, 9, nullptr, nullptr, nullptr, nullptr), 0, "");
    EXPECT(rf_recover_forward_f32(nullptr, f, 10, q, 5, 0, f, f, f, nullptr), -1, "NULL pointer");
    EXPECT(rf_recover_forward_f32(f, f, -1, q, 5, 0, f, f, f, nullptr), -1, "bad size");
    EXPECT(rf_recover_forward_f32(f, f, 10, q, 1ll << 31, 0, f, f, f, nullptr), -2, "too many pixels");
    EXPECT(rf_recover_forward_f32(f, f, 10, q, 5, 4, f, f, f, nullptr), -1, "unknown norm");
    EXPECT(rf_recover_forward_f32(f, f, 10, nullptr, 11, 0, f, f, f, nullptr), -1, "without a pixel list");
    EXPECT(rf_recover_boundary_plan(1000, nullptr), -1, "NULL pointer");
    EXPECT(rf_recover_boundary_plan(1000, plan), 0, "");
    EXPECT(rf_recover_boundary_plan(1ll << 31, plan), -2, "too many pixels");
    EXPECT(rf_recover_boundary_backward_f32(nullptr, nullptr, 0, 9, 9, nan, nan, nullptr, nullptr, nullptr, 0, nullptr), 0, "");
    EXPECT(rf_recover_boundary_backward_f32(f, f, 1000, 0, 1, .1f, .1f, nullptr, f, ws, need, nullptr), -1, "NULL pointer");
    EXPECT(rf_recover_boundary_backward_f32(f, f, 1000, 0, 3, .1f, .1f, d, f, ws, need, nullptr), -1, "unknown penalty");
    EXPECT(rf_recover_boundary_backward_f32(f, f, 1000, -1, 1, .1f, .1f, d, f, ws, need, nullptr), -1, "unknown norm");
    EXPECT(rf_recover_boundary_backward_f32(f, f, 1000, 0, 1, nan, .1f, d, f, ws, need, nullptr), -1, "finite");
    EXPECT(rf_recover_boundary_backward_f32(f, f, 1000, 0, 1, .1f, inf, d, f, ws, need, nullptr), -1, "finite");
    EXPECT(rf_recover_boundary_backward_f32(f, f, 1000, 0, 1, .1f, .1f, d, f, ws, need - 1, nullptr), -1, "16-byte aligned");
    EXPECT(rf_recover_boundary_backward_f32(f, f, 1000, 0, 1, .1f, .1f, d, f, (void *)0x1008, need, nullptr), -1, "16-byte aligned");
    EXPECT(rf_recover_boundary_backward_f32(f, f, 1000, 0, 1, .1f, .1f, d, f, nullptr, need, nullptr), -1, "16-byte aligned");
    EXPECT(rf_recover_boundary_backward_f32(f, f, 1ll << 31, 0, 1, .1f, .1f, d, f, ws, need, nullptr), -2, "too many pixels");
    EXPECT(rf_recover_hinge_scatter_f32(nullptr, nullptr, nullptr, nullptr, 0, 10, 9, nan, nullptr, nullptr), 0, "");
    EXPECT(rf_recover_hinge_scatter_f32(f, f, f, nullptr, 5, 10, 0, 1.f, f, nullptr), -1, "NULL pointer");
    EXPECT(rf_recover_hinge_scatter_f32(f, f, f, q, -5, 10, 0, 1.f, f, nullptr), -1, "bad size");
    EXPECT(rf_recover_hinge_scatter_f32(f, f, f, q, 5, 1ll << 31, 0, 1.f, f, nullptr), -2, "too many pixels");
    EXPECT(rf_recover_hinge_scatter_f32(f, f, f, q, 5, 10, 7, 1.f, f, nullptr), -1, "unknown norm");
    EXPECT(rf_recover_hinge_scatter_f32(f, f, f, q, 5, 10, 0, nan, f, nullptr), -1, "finite");
    printf("%d failures\n", failures);
    return failures != 0;
}
