// experiment: what separates two consecutive full-chip kernels -- the queue they share, or the event the first one carries?
// (the ~10 us between consecutive layer-1 launches of the role pipeline.)
//
// A chain of kernels with the one-launch layer 1's footprint (256 threads, __launch_bounds__(256, 3), ~160 VGPRs, 41 KB LDS; 768 blocks =
// every slot of a 256-CU part), each block busy for a fixed time on the wall clock, launched
//   way 0: on one stream, plain launches;
//   way 1: on one stream, every launch carrying a stop event through hipExtLaunchKernelGGL (untimed, no system fence: the role
//          pipeline's hand-off event, csrc/sage_internal.h sage_launch);
//   way 2: alternating over two streams, plain launches, no dependency between the streams;
//   way 3: alternating over two streams, every launch carrying a stop event (what alternating layer-1 streams would do);
//   way 4: on one stream, every launch carrying its own TIMED start and stop events (the profiled submit): the gaps are then also read
//          from the events, to set the two clocks against each other;
// on an idle chip, or beside a resident latency-bound grid (one 64-thread wave per CU chasing pointers) on a third stream.
// Every kernel stamps the wall clock: atomicMin of its blocks' first instruction, atomicMax of their last.  Reported per way:
// start(i + 1) - end(i) over the chain, and the kernel's own duration.
#include <hip/hip_ext.h>
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s -> %s\n", #x, hipGetErrorString(e_)); return -1; } } while (0)

enum { kAcc = 150, kLdsFloats = 41 * 256, kMaxChain = 64 };

// busy for `ticks` of the wall clock (bounded by `max_rounds` whatever the clock says)
extern "C" __global__ void __launch_bounds__(256, 3) k_footprint(unsigned long long* stamps, long long ticks, int max_rounds, float* sink) {
    __shared__ float lds[kLdsFloats];
    const unsigned long long t0 = wall_clock64();
    if (threadIdx.x == 0) atomicMin(&stamps[0], t0);
    float acc[kAcc];
#pragma unroll
    for (int i = 0; i < kAcc; ++i) acc[i] = (float)(threadIdx.x + i);
    for (int i = threadIdx.x; i < kLdsFloats; i += 256) lds[i] = (float)i;
    __syncthreads();
    for (int r = 0; r < max_rounds; ++r) {
        const float x = lds[(threadIdx.x * 33 + r) % kLdsFloats];
#pragma unroll
        for (int i = 0; i < kAcc; ++i) acc[i] = fmaf(acc[i], 1.0001f, x);
        if ((long long)(wall_clock64() - t0) >= ticks) break;
    }
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < kAcc; ++i) s += acc[i];
    if (s == 12345.678f) sink[0] = s;                       // keeps the accumulators alive; never true in practice
    __syncthreads();
    if (threadIdx.x == 0) atomicMax(&stamps[1], wall_clock64());
}

// the company: one wave per block, dependent loads through a small L2-resident ring until the wall clock says stop
extern "C" __global__ void __launch_bounds__(64) k_company(const int* __restrict__ next, long long ticks, int max_rounds, int* sink) {
    const unsigned long long t0 = wall_clock64();
    int i = (blockIdx.x * 64 + threadIdx.x) & 1023;
    for (int r = 0; r < max_rounds; ++r) {
        for (int d = 0; d < 16; ++d) i = next[i];
        if ((long long)(wall_clock64() - t0) >= ticks) break;
    }
    if (i == -1) *sink = i;
}

// One chain.  gaps_us[n - 1], durations_us[n]: from the kernels' stamps; event_gaps_us[n - 1]: way 4 only (else untouched).  -> 0 / -1
extern "C" int run_boundary(int way, int beside, int n, double kernel_us, double* gaps_us, double* durations_us, double* event_gaps_us) {
    if (n < 2 || n > kMaxChain || way < 0 || way > 4 || kernel_us <= 0 || kernel_us > 1000) return -1;
    int khz = 0, cus = 0;
    CHECK(hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, 0));
    CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, 0));
    if (khz <= 0) return -1;
    const double ticks_per_us = khz / 1e3;
    hipStream_t st[3];
    for (auto& s : st) CHECK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    unsigned long long* stamps = nullptr;
    unsigned long long init[2 * kMaxChain], got[2 * kMaxChain];
    for (int i = 0; i < n; ++i) { init[2 * i] = ~0ull; init[2 * i + 1] = 0; }
    CHECK(hipMalloc(&stamps, sizeof(init)));
    CHECK(hipMemcpy(stamps, init, sizeof(init), hipMemcpyHostToDevice));
    float* sink = nullptr;
    CHECK(hipMalloc(&sink, 256));
    int* ring = nullptr;
    int ring_host[1024];
    for (int i = 0; i < 1024; ++i) ring_host[i] = (i * 397 + 1) & 1023;
    CHECK(hipMalloc(&ring, sizeof(ring_host)));
    CHECK(hipMemcpy(ring, ring_host, sizeof(ring_host), hipMemcpyHostToDevice));
    hipEvent_t stop[kMaxChain], t_start[kMaxChain], t_stop[kMaxChain];
    for (int i = 0; i < n; ++i) {
        CHECK(hipEventCreateWithFlags(&stop[i], hipEventDisableTiming | hipEventDisableSystemFence));
        CHECK(hipEventCreate(&t_start[i]));
        CHECK(hipEventCreate(&t_stop[i]));
    }
    const long long ticks = (long long)(kernel_us * ticks_per_us);
    const int rounds_cap = 1 << 22;                          // seconds of work at most, whatever the clock does
    const dim3 grid(3 * cus), block(256);
    // warm the code objects and both streams
    for (int s = 0; s < 2; ++s) hipLaunchKernelGGL(k_footprint, grid, block, 0, st[s], stamps, (long long)(2 * ticks_per_us), rounds_cap, sink);
    hipLaunchKernelGGL(k_company, dim3(1), dim3(64), 0, st[2], ring, (long long)(2 * ticks_per_us), rounds_cap, (int*)sink);
    CHECK(hipDeviceSynchronize());
    CHECK(hipMemcpy(stamps, init, sizeof(init), hipMemcpyHostToDevice));
    if (beside)                                              // resident for the whole chain, and a little longer
        hipLaunchKernelGGL(k_company, dim3(cus), dim3(64), 0, st[2], ring, (long long)((n + 4) * kernel_us * ticks_per_us), rounds_cap, (int*)sink);
    for (int i = 0; i < n; ++i) {
        hipStream_t s = (way == 2 || way == 3) ? st[i & 1] : st[0];
        unsigned long long* my = stamps + 2 * i;
        if (way == 1 || way == 3)
            hipExtLaunchKernelGGL(k_footprint, grid, block, 0, s, nullptr, stop[i], 0u, my, ticks, rounds_cap, sink);
        else if (way == 4)
            hipExtLaunchKernelGGL(k_footprint, grid, block, 0, s, t_start[i], t_stop[i], 0u, my, ticks, rounds_cap, sink);
        else
            hipLaunchKernelGGL(k_footprint, grid, block, 0, s, my, ticks, rounds_cap, sink);
    }
    CHECK(hipDeviceSynchronize());
    CHECK(hipMemcpy(got, stamps, sizeof(got), hipMemcpyDeviceToHost));
    for (int i = 0; i < n; ++i) durations_us[i] = (double)(got[2 * i + 1] - got[2 * i]) / ticks_per_us;
    for (int i = 0; i + 1 < n; ++i) gaps_us[i] = (double)((long long)(got[2 * i + 2] - got[2 * i + 1])) / ticks_per_us;
    if (way == 4)
        for (int i = 0; i + 1 < n; ++i) {
            float ms = 0.f;
            CHECK(hipEventElapsedTime(&ms, t_stop[i], t_start[i + 1]));
            event_gaps_us[i] = 1e3 * ms;
        }
    for (int i = 0; i < n; ++i) { (void)hipEventDestroy(stop[i]); (void)hipEventDestroy(t_start[i]); (void)hipEventDestroy(t_stop[i]); }
    (void)hipFree(stamps); (void)hipFree(sink); (void)hipFree(ring);
    for (auto& s : st) (void)hipStreamDestroy(s);
    return 0;
}
