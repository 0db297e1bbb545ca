// What the full-neighbourhood mean (sage_csr_mean.hip) and its backward (sage_csr_mean_backward.hip) share: the clamped row span,
// the small vector helpers, and the three launches that cut long rows into chunks of SAGE_CSR_MEAN_CHUNK edges
// (count -> carry -> expand; see the head of sage_csr_mean.hip).  Everything has internal linkage: each translation unit that
// includes this holds its own copy of the kernels.
#pragma once
#include "sage_internal.h"

#include <algorithm>

namespace {

constexpr int64_t kChunk = SAGE_CSR_MEAN_CHUNK;
constexpr int kCountThreads = 256, kCountIpt = 8, kCountTile = kCountThreads * kCountIpt;
constexpr int kCarryThreads = 1024;

size_t align256(size_t x) { return (x + 255) / 256 * 256; }

template <int VEC> struct VecT;
template <> struct VecT<4> { using type = float4; };
template <> struct VecT<1> { using type = float; };

__device__ inline void vadd(float4& a, const float4& b) { a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w; }
__device__ inline void vadd(float& a, const float& b) { a += b; }
__device__ inline float4 vscale(const float4& a, float s) { return make_float4(a.x * s, a.y * s, a.z * s, a.w * s); }
__device__ inline float vscale(const float& a, float s) { return a * s; }
__device__ inline void vfill(float4& a, float s) { a = make_float4(s, s, s, s); }
__device__ inline void vfill(float& a, float s) { a = s; }

__device__ inline int64_t uniform64(int64_t x) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)x);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)((uint64_t)x >> 32));
    return (int64_t)(((uint64_t)hi << 32) | lo);
}

// Row r's node and edge range, clamped: a node id outside [0, num_nodes) is an empty row without a self term (v = -1),
// row pointers are clamped into [0, rowptr[num_nodes]] and made non-decreasing, so no edge index leaves col[].
__device__ inline void row_span(const int64_t* __restrict__ rowptr, int64_t num_nodes, const int32_t* __restrict__ nodes, int r,
                                int64_t total, int32_t& v, int64_t& b, int64_t& e) {
    v = nodes ? nodes[r] : r;
    if (v < 0 || (int64_t)v >= num_nodes) { v = -1; b = e = 0; return; }
    b = rowptr[v];
    e = rowptr[v + 1];
    b = min(max(b, (int64_t)0), total);
    e = min(max(e, b), total);
}

__device__ inline int64_t long_chunks(int64_t deg) { return deg > kChunk ? (deg + kChunk - 1) / kChunk : 0; }

// 1. per-thread kCountIpt consecutive rows; off[r] := block-local exclusive offset, carry[block] := the block's chunk sum
__global__ __launch_bounds__(kCountThreads) void csr_count_kernel(const int64_t* __restrict__ rowptr, int64_t num_nodes,
                                                                   const int32_t* __restrict__ nodes, int n, int64_t* __restrict__ off,
                                                                   int64_t* __restrict__ carry) {
    __shared__ int64_t wave_sum[kCountThreads / kWave];
    const int64_t total = rowptr[num_nodes];
    const int r0 = blockIdx.x * kCountTile + threadIdx.x * kCountIpt;
    int64_t c[kCountIpt], s = 0;
#pragma unroll
    for (int i = 0; i < kCountIpt; ++i) {
        c[i] = 0;
        if (r0 + i < n) {
            int32_t v;
            int64_t b, e;
            row_span(rowptr, num_nodes, nodes, r0 + i, total, v, b, e);
            c[i] = long_chunks(e - b);
        }
        s += c[i];
    }
    // block exclusive scan of the thread sums: within the wave by shuffles, then across the 4 waves
    const int lane = sage_lane(), w = threadIdx.x / kWave;
    int64_t incl = s;
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
        const int64_t y = __shfl_up(incl, d, kWave);
        if (lane >= d) incl += y;
    }
    if (lane == kWave - 1) wave_sum[w] = incl;
    __syncthreads();
    int64_t before = 0, block = 0;
#pragma unroll
    for (int i = 0; i < kCountThreads / kWave; ++i) {
        if (i < w) before += wave_sum[i];
        block += wave_sum[i];
    }
    int64_t run = before + incl - s;
#pragma unroll
    for (int i = 0; i < kCountIpt; ++i) {
        if (r0 + i < n) off[r0 + i] = run;
        run += c[i];
    }
    if (threadIdx.x == 0) carry[blockIdx.x] = block;
}

// 2. one block: carry[0..nb) := exclusive scan of itself, carry[nb] := total chunks
__global__ __launch_bounds__(kCarryThreads) void csr_carry_kernel(int64_t* __restrict__ carry, int nb) {
    __shared__ int64_t wave_sum[kCarryThreads / kWave];
    __shared__ int64_t base_sh;
    const int lane = sage_lane(), w = threadIdx.x / kWave;
    if (threadIdx.x == 0) base_sh = 0;
    __syncthreads();
    for (int t0 = 0; t0 < nb; t0 += kCarryThreads) {
        const int i = t0 + threadIdx.x;
        const int64_t x = i < nb ? carry[i] : 0;
        int64_t incl = x;
#pragma unroll
        for (int d = 1; d < kWave; d <<= 1) {
            const int64_t y = __shfl_up(incl, d, kWave);
            if (lane >= d) incl += y;
        }
        if (lane == kWave - 1) wave_sum[w] = incl;
        __syncthreads();
        int64_t before = base_sh, tile = 0;
        for (int j = 0; j < kCarryThreads / kWave; ++j) {
            if (j < w) before += wave_sum[j];
            tile += wave_sum[j];
        }
        if (i < nb) carry[i] = before + incl - x;
        __syncthreads();                               // every thread has read base_sh and wave_sum
        if (threadIdx.x == 0) base_sh += tile;
        __syncthreads();
    }
    if (threadIdx.x == 0) carry[nb] = base_sh;
}

// 3. off[r] := global chunk offset; the chunks of a long row that fit the workspace get item entries
__global__ __launch_bounds__(256) void csr_expand_kernel(const int64_t* __restrict__ rowptr, int64_t num_nodes,
                                                         const int32_t* __restrict__ nodes, int n, int64_t* __restrict__ off,
                                                         const int64_t* __restrict__ carry, int64_t cap, int32_t* __restrict__ item_row) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    const int64_t total = rowptr[num_nodes];
    int32_t v;
    int64_t b, e;
    row_span(rowptr, num_nodes, nodes, r, total, v, b, e);
    const int64_t k = long_chunks(e - b);
    const int64_t o = off[r] + carry[r / kCountTile];
    off[r] = o;
    if (k > 0 && o + k <= cap)
        for (int64_t c = 0; c < k; ++c) item_row[o + c] = r;
}

// Item entries (= partial rows) a workspace sized for max_edges holds: the chunks of all long rows are at most
// floor(E_sel / E) + (number of long rows), and a long row has more than E edges.
inline int64_t csr_item_cap(int32_t n, int64_t max_edges) { return max_edges / kChunk + std::min<int64_t>(n, max_edges / (kChunk + 1)); }

}  // namespace
