// Scalar-unit calibration for the replay's issue arithmetic: kernels of a known
// instruction mix, run with W waves on every SIMD of every CU, timed, and counted under
// rocprofv3 --pmc (SQ_INSTS_SALU / SQ_INSTS_VALU / SQ_INSTS_BRANCH, in a run of its own).
//   mode 0  salu     64 independent s_add_u32 per iteration
//   mode 1  nop      64 s_nop 0 per iteration
//   mode 2  waitcnt  64 s_waitcnt lgkmcnt(0) per iteration (nothing outstanding)
//   mode 3  valu     64 independent v_add_u32 per iteration (wave64)
//   mode 4  mix      32 s_add_u32 interleaved with 32 v_add_u32 per iteration
//   mode 5  branch   64 taken s_branch (to the next instruction) per iteration
// Every iteration also holds the loop's own s_add / s_cmp / s_cbranch (3 scalar instructions,
// printed as "expected").  What the timing gives is instructions per CU per nanosecond at each
// occupancy, so the replay's scalar instructions per CU per nanosecond can be set against the
// unit's measured peak without assuming a clock or an issue rule.
// Build: hipcc -O3 --offload-arch=gfx950 -o tools/salu_unit_probe tools/salu_unit_probe.hip
// Run:   tools/salu_unit_probe [mode waves_per_simd]    (no arguments: the whole table)
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>

#define R4(x) x x x x
#define R16(x) R4(x) R4(x) R4(x) R4(x)

template <int MODE>
__global__ __launch_bounds__(256) void probe(int iters, unsigned *sink) {
    unsigned s0 = 1, s1 = 2, s2 = 3, s3 = 4;
    unsigned v0 = threadIdx.x, v1 = 1, v2 = 2, v3 = 3;
    for (int i = 0; i < iters; i++) {
        if (MODE == 0)
            asm volatile(R16("s_add_u32 %0, %0, 1\n s_add_u32 %1, %1, 1\n s_add_u32 %2, %2, 1\n s_add_u32 %3, %3, 1\n")
                         : "+s"(s0), "+s"(s1), "+s"(s2), "+s"(s3) : : "scc");
        if (MODE == 1) asm volatile(R16(R4("s_nop 0\n")));
        if (MODE == 2) asm volatile(R16(R4("s_waitcnt lgkmcnt(0)\n")));
        if (MODE == 3)
            asm volatile(R16("v_add_u32 %0, %0, 1\n v_add_u32 %1, %1, 1\n v_add_u32 %2, %2, 1\n v_add_u32 %3, %3, 1\n")
                         : "+v"(v0), "+v"(v1), "+v"(v2), "+v"(v3));
        if (MODE == 4)
            asm volatile(R16("s_add_u32 %0, %0, 1\n v_add_u32 %2, %2, 1\n s_add_u32 %1, %1, 1\n v_add_u32 %3, %3, 1\n")
                         : "+s"(s0), "+s"(s1), "+v"(v0), "+v"(v1) : : "scc");
        if (MODE == 5) asm volatile(R16(R4("s_branch 0\n")));
    }
    if (s0 + s1 + s2 + s3 + v0 + v1 + v2 + v3 == 0xFFFFFFFFu) sink[0] = 1;   // keeps the chains alive
}

typedef void (*Kern)(int, unsigned *);
static const Kern kerns[] = {probe<0>, probe<1>, probe<2>, probe<3>, probe<4>, probe<5>};
static const char *names[] = {"salu", "nop", "waitcnt", "valu", "mix", "branch"};

static void run(int mode, int w, int n_cu, unsigned *sink) {
    const int iters = 20000;
    hipEvent_t a, b;
    (void)hipEventCreate(&a);
    (void)hipEventCreate(&b);
    // a 256-thread workgroup is four waves, one per SIMD: n_cu * w of them fill w waves per SIMD
    hipLaunchKernelGGL(kerns[mode], dim3(n_cu * w), dim3(256), 0, 0, 100, sink);   // warm
    (void)hipEventRecord(a);
    hipLaunchKernelGGL(kerns[mode], dim3(n_cu * w), dim3(256), 0, 0, iters, sink);
    (void)hipEventRecord(b);
    (void)hipEventSynchronize(b);
    float ms = 0;
    (void)hipEventElapsedTime(&ms, a, b);
    (void)hipEventDestroy(a);
    (void)hipEventDestroy(b);
    const double body = double(iters) * 64, loop = double(iters) * 3;
    const double s_body = mode == 3 ? 0 : mode == 4 ? body / 2 : body, v_body = mode == 3 ? body : mode == 4 ? body / 2 : 0;
    printf("%-8s waves/SIMD %d  %8.3f ms  expected per wave: scalar %.0f (+%.0f loop) vector %.0f;"
           "  per CU per ns: scalar %.3f vector %.3f\n",
           names[mode], w, ms, s_body, loop, v_body, (s_body + loop) * w * 4 / (ms * 1e6), v_body * w * 4 / (ms * 1e6));
}

int main(int argc, char **argv) {
    hipDeviceProp_t p;
    if (hipGetDeviceProperties(&p, 0) != hipSuccess) { fprintf(stderr, "no HIP device\n"); return 1; }
    const int n_cu = p.multiProcessorCount;
    unsigned *sink;
    (void)hipMalloc(&sink, 4);
    printf("%s (%s): %d CUs, clock %.0f MHz\n", p.name[0] ? p.name : "device 0", p.gcnArchName, n_cu, p.clockRate / 1e3);
    if (argc >= 3) {
        run(atoi(argv[1]) % 6, atoi(argv[2]), n_cu, sink);
    } else {
        for (int mode = 0; mode < 6; mode++)
            for (int w : {1, 2, 4, 8}) run(mode, w, n_cu, sink);
    }
    const bool ok = hipDeviceSynchronize() == hipSuccess;
    (void)hipFree(sink);
    return ok ? 0 : 1;
}
