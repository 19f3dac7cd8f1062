// msad_overlap.hip -- issue cost of v_msad_u8 (gfx950) set against v_sad_u8, measured the way
// pipe_overlap.hip measured the SAD: back to back, and as a pair with a two-cycle v_mul_f32 /
// v_add_f32 on VGPRs and with the SGPR-operand v_mul_f32 of the joint bilateral tap loop.  Decides
// whether the masked SAD may replace {v_and_b32, v_sad_u8} in that loop (rf_jbf_taploops.hpp): it
// pays only if a pair with v_msad_u8 costs what the pair with v_sad_u8 costs.
// 8 independent chains per wave: a figure is an ISSUE cost, not a dependent latency.
// Build: hipcc -O3 --offload-arch=gfx950 msad_overlap.hip -o msad_overlap.bin
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>

#define CHECK(x)                                                           \
    do {                                                                   \
        hipError_t e = (x);                                                \
        if (e != hipSuccess) {                                             \
            fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e));         \
            exit(1);                                                       \
        }                                                                  \
    } while (0)

constexpr int kIters = 4096 * 32;

#define OPS4(OP) OP(r0) OP(r0) OP(r0) OP(r0)

#define KERNEL(NAME, ASM)                                                                  \
    __global__ void NAME(unsigned *out, int iters, unsigned long long *clk)                \
    {                                                                                      \
        extern __shared__ unsigned dyn_lds[];                                              \
        if (iters < 0)                                                                     \
            dyn_lds[threadIdx.x] = 1;                                                      \
        unsigned r0 = threadIdx.x * 2654435761u, r1 = r0 ^ 0x55, r2 = r0 + 77, r3 = r0 * 3, \
                 r4 = r0 + 5, r5 = r0 ^ 9, r6 = r0 + 11, r7 = r0 * 7;                       \
        const unsigned a = threadIdx.x | 0x01020304u, b = 0x3f800001u;                     \
        unsigned long long t0 = __builtin_amdgcn_s_memtime();                              \
        unsigned long long q0 = __builtin_amdgcn_s_memrealtime();                          \
        for (int it = 0; it < iters; it++) {                                               \
            OPS4(ASM)                                                                      \
        }                                                                                  \
        unsigned long long t1 = __builtin_amdgcn_s_memtime();                              \
        unsigned long long q1 = __builtin_amdgcn_s_memrealtime();                          \
        if (blockIdx.x == 0 && threadIdx.x == 0 && clk) {                                  \
            clk[0] = t1 - t0;                                                              \
            clk[1] = q1 - q0;                                                              \
        }                                                                                  \
        unsigned r = r0 + r1 + r2 + r3 + r4 + r5 + r6 + r7;                                \
        if (r == 0x12345678u)                                                              \
            out[threadIdx.x] = r;                                                          \
    }

// operand %8 = a (VGPR, every byte non-zero in byte 0..3 for most lanes), %9 = b (VGPR), %10 = b (SGPR)
#define REGS "+v"(r0), "+v"(r1), "+v"(r2), "+v"(r3), "+v"(r4), "+v"(r5), "+v"(r6), "+v"(r7) : "v"(a), "v"(b), "s"(b)
#define F_SAD(x) "v_sad_u8 %" #x ", %" #x ", %8, 0\n"
#define F_MSAD(x) "v_msad_u8 %" #x ", %" #x ", %8, 0\n"
#define S_MUL(x) "v_mul_f32 %" #x ", %9, %" #x "\n"
#define S_ADD(x) "v_add_f32 %" #x ", %9, %" #x "\n"
#define S_AND(x) "v_and_b32 %" #x ", %9, %" #x "\n"
#define F_MULS(x) "v_mul_f32 %" #x ", %10, %" #x "\n"
// 16 instructions per OP: 8 X + 8 Y interleaved one for one, on disjoint chains
#define INTER(X, Y) asm volatile(X(0) Y(1) X(2) Y(3) X(4) Y(5) X(6) Y(7) X(1) Y(0) X(3) Y(2) X(5) Y(4) X(7) Y(6) : REGS);
#define ONLY(X) asm volatile(X(0) X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(0) X(1) X(2) X(3) X(4) X(5) X(6) X(7) : REGS);
#define A_ONLY_SAD(u_) ONLY(F_SAD)
#define A_ONLY_MSAD(u_) ONLY(F_MSAD)
#define A_SAD_MUL(u_) INTER(F_SAD, S_MUL)
#define A_MSAD_MUL(u_) INTER(F_MSAD, S_MUL)
#define A_SAD_ADD(u_) INTER(F_SAD, S_ADD)
#define A_MSAD_ADD(u_) INTER(F_MSAD, S_ADD)
#define A_SAD_MULS(u_) INTER(F_SAD, F_MULS)
#define A_MSAD_MULS(u_) INTER(F_MSAD, F_MULS)
#define A_AND_MUL(u_) INTER(S_AND, S_MUL)
KERNEL(k_only_sad, A_ONLY_SAD)
KERNEL(k_only_msad, A_ONLY_MSAD)
KERNEL(k_sad_mul, A_SAD_MUL)
KERNEL(k_msad_mul, A_MSAD_MUL)
KERNEL(k_sad_add, A_SAD_ADD)
KERNEL(k_msad_add, A_MSAD_ADD)
KERNEL(k_sad_mulsgpr, A_SAD_MULS)
KERNEL(k_msad_mulsgpr, A_MSAD_MULS)
KERNEL(k_and_mul, A_AND_MUL)

typedef void (*kern_t)(unsigned *, int, unsigned long long *);

void run(const char *name, kern_t k, unsigned *d_out, unsigned long long *d_clk)
{
    hipEvent_t e0, e1;
    CHECK(hipEventCreate(&e0));
    CHECK(hipEventCreate(&e1));
    for (int wps : {1, 4, 8}) {
        // 256-thread blocks (one wave per SIMD each); LDS per block caps blocks/CU = waves/SIMD;
        // 16 rounds of blocks per CU so that placement imbalance averages out
        const int threads = 256;
        const int blocks = 256 * wps * 16;
        const size_t lds = (160 * 1024) / wps - (wps > 1 ? 1024 : 0);
        CHECK(hipFuncSetAttribute((const void *)k, hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)lds));
        hipLaunchKernelGGL(k, dim3(blocks), dim3(threads), lds, 0, d_out, kIters / 64, nullptr);
        CHECK(hipDeviceSynchronize());
        CHECK(hipEventRecord(e0));
        hipLaunchKernelGGL(k, dim3(blocks), dim3(threads), lds, 0, d_out, kIters / 16, d_clk);
        CHECK(hipEventRecord(e1));
        CHECK(hipEventSynchronize(e1));
        float ms = 0;
        CHECK(hipEventElapsedTime(&ms, e0, e1));
        unsigned long long clk[2];
        CHECK(hipMemcpy(clk, d_clk, sizeof(clk), hipMemcpyDeviceToHost));
        const double ghz = (double)clk[0] / ((double)clk[1] * 10.0);  // realtime ticks are 100 MHz
        const double winstr = (double)(kIters / 16) * 4 * 16;         // per wave
        const double per_simd = winstr * 16.0 * wps;                  // 16 rounds x wps waves per SIMD
        const double cyc = ms * 1e-3 * ghz * 1e9 / per_simd;
        printf("%-18s waves/SIMD=%d %8.3f ms  clock(blk0) %.3f GHz  %.2f cycles/wave-instr/SIMD  "
               "%.2f cycles/pair\n", name, wps, ms, ghz, cyc, 2.0 * cyc);
    }
}

int main()
{
    unsigned *d_out;
    unsigned long long *d_clk;
    CHECK(hipMalloc(&d_out, 1 << 16));
    CHECK(hipMalloc(&d_clk, 64));
    for (int i = 0; i < 10; i++)
        hipLaunchKernelGGL(k_only_sad, dim3(1024), dim3(256), 0, 0, d_out, kIters / 16, nullptr);
    CHECK(hipDeviceSynchronize());
#define RUN(k) run(#k, k, d_out, d_clk)
    RUN(k_only_sad);
    RUN(k_only_msad);
    RUN(k_sad_mul);
    RUN(k_msad_mul);
    RUN(k_sad_add);
    RUN(k_msad_add);
    RUN(k_sad_mulsgpr);
    RUN(k_msad_mulsgpr);
    RUN(k_and_mul);
    return 0;
}
