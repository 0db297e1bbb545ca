// Terms sorted by destination row, behind sage_embed_grad.hip and sage_csr_mean_backward_rows.hip: int32 (key, value) pairs with keys in
// [0, rows] (rows = the sentinel of an unused slot), a STABLE hipcub radix sort on the key bits that matter, so the order the terms
// were laid out in survives inside a run of equal keys, and over the sorted keys either a row pointer (one entry per row) or a run
// list (one entry per row that has a term: the _rows / _touched entries, which size nothing by `rows`).  The sort's temporary is reserved by
// host arithmetic (a workspace size query must answer without a device) and checked against the library before the sort.
#pragma once
#include <hipcub/hipcub.hpp>

#include "sage_csr_common.h"

namespace {

// Bits that tell the keys 0 .. rows apart.
inline int sort_key_bits(int64_t rows) {
    int bits = 1;
    while ((1ll << bits) <= rows) ++bits;
    return bits;
}

// Bytes reserved for the temporary of a sort of `slots` pairs (see sort_ws in sage_embed_grad.hip for what the bound covers).
inline size_t sort_temp_reserve(int64_t slots) { return (size_t)slots * 16 + 65536; }

inline hipError_t sort_temp_bytes(int slots, int bits, size_t* bytes) {
    *bytes = 0;
    return hipcub::DeviceRadixSort::SortPairs(nullptr, *bytes, (const int32_t*)nullptr, (int32_t*)nullptr, (const int32_t*)nullptr,
                                              (int32_t*)nullptr, slots, 0, bits, (hipStream_t)0);
}

// rowptr[e] = the first position of the sorted list whose key is >= e, e in [0, rows]: rowptr[rows] = the terms
__global__ __launch_bounds__(256) void sorted_rowptr_kernel(const int32_t* __restrict__ keys, int slots, int rows,
                                                            int64_t* __restrict__ rowptr) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e > rows) return;
    int lo = 0, hi = slots;
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        if (keys[mid] < e) lo = mid + 1;
        else hi = mid;
    }
    rowptr[e] = lo;
}

// ---- the run list of the sorted keys: what takes the place of the row pointer where nothing may be sized by `rows` ------------------
// The sorted keys are the rows with a term, ascending, each a run of equal keys, then the sentinels.  Run u = (run_row[u],
// [runptr[u], runptr[u + 1])), u < U; entries [U, runs_cap] of runptr hold the end of the terms (empty spans), so csr_chunk_plan and
// the chunk kernels walk the list as they walk a CSR of runs_cap rows.  runs_cap = min(slots, rows) bounds U on the host.
constexpr int kHeadThreads = 256, kHeadIpt = 8, kHeadTile = kHeadThreads * kHeadIpt;

// Is position i of the sorted keys the first of a run of a row (the sentinel's run is none)?
__device__ inline bool run_head(const int32_t* __restrict__ keys, int64_t i, int sentinel) {
    const int key = keys[i];
    return key != sentinel && (i == 0 || keys[i - 1] != key);
}

// 3a / 3c. kHeadIpt consecutive positions per thread.  SCATTER false: heads[block] := the run heads in the block's tile (then
// csr_carry_kernel: heads[block] := the runs before the tile, heads[head_blocks] := U).  SCATTER true: run u = heads[block] + (the
// heads before it in the tile) gets its row and its start, and the one position where the terms end (the first sentinel, or
// slots) is written to end_pos
template <bool SCATTER>
__global__ __launch_bounds__(kHeadThreads) void embed_heads_kernel(const int32_t* __restrict__ keys, int slots, int sentinel, int64_t runs_cap,
                                                                    int64_t* __restrict__ heads, int32_t* __restrict__ run_row,
                                                                    int64_t* __restrict__ runptr, int64_t* __restrict__ end_pos) {
    __shared__ int wave_sum[kHeadThreads / kWave];
    const int64_t i0 = (int64_t)blockIdx.x * kHeadTile + (int64_t)threadIdx.x * kHeadIpt;
    bool h[kHeadIpt];
    int s = 0;
#pragma unroll
    for (int u = 0; u < kHeadIpt; ++u) {
        h[u] = i0 + u < slots && run_head(keys, i0 + u, sentinel);
        s += h[u] ? 1 : 0;
    }
    const int lane = sage_lane(), w = threadIdx.x / kWave;
    int incl = s;
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
        const int y = __shfl_up(incl, d, kWave);
        if (lane >= d) incl += y;
    }
    if (lane == kWave - 1) wave_sum[w] = incl;
    __syncthreads();
    int before = 0, block = 0;
#pragma unroll
    for (int i = 0; i < kHeadThreads / kWave; ++i) {
        if (i < w) before += wave_sum[i];
        block += wave_sum[i];
    }
    if (!SCATTER) {
        if (threadIdx.x == 0) heads[blockIdx.x] = block;
        return;
    }
    int64_t u_run = heads[blockIdx.x] + before + incl - s;
#pragma unroll
    for (int u = 0; u < kHeadIpt; ++u) {
        const int64_t i = i0 + u;
        if (i >= slots) break;
        if (h[u]) {
            if (u_run < runs_cap) {                                  // always: distinct keys below the sentinel are at most runs_cap
                run_row[u_run] = keys[i];
                runptr[u_run] = i;
            }
            ++u_run;
        }
        const int key = keys[i];
        if (key == sentinel && (i == 0 || keys[i - 1] != sentinel)) *end_pos = i;          // sorted: exactly one such position, or none
        if (i == slots - 1 && key != sentinel) *end_pos = slots;
    }
}

// 3d. runptr[u] := the end of the terms for u in [U, runs_cap]; num_rows_out[0] := U
__global__ __launch_bounds__(256) void embed_runs_fill_kernel(const int64_t* __restrict__ heads, int head_blocks, const int64_t* __restrict__ end_pos,
                                                              int64_t runs_cap, int64_t* __restrict__ runptr, int32_t* __restrict__ num_rows_out) {
    const int64_t u = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t nruns = min(heads[head_blocks], runs_cap);
    if (u == 0) num_rows_out[0] = (int32_t)nruns;
    if (u >= nruns && u <= runs_cap) runptr[u] = *end_pos;
}

// The run list of `slots` sorted keys (sentinel = rows): count the heads per tile, scan the tiles, write the runs, close the list.
// heads holds head_blocks(slots) + 1 entries; afterwards heads[head_blocks] = U, which is also stored to num_rows_out[0].
inline int64_t run_head_blocks(int64_t slots) { return (slots + kHeadTile - 1) / kHeadTile; }

inline int sorted_run_list(const int32_t* keys, int slots, int sentinel, int64_t runs_cap, int64_t* heads, int32_t* run_row, int64_t* runptr,
                           int64_t* end_pos, int32_t* num_rows_out, hipStream_t st) {
    const int hb = (int)run_head_blocks(slots);
    hipLaunchKernelGGL(embed_heads_kernel<false>, dim3(hb), dim3(kHeadThreads), 0, st, keys, slots, sentinel, runs_cap, heads, run_row, runptr,
                       end_pos);
    SAGE_CHECK_LAUNCH("embed_heads_kernel (count)");
    hipLaunchKernelGGL(csr_carry_kernel, dim3(1), dim3(kCarryThreads), 0, st, heads, hb);
    SAGE_CHECK_LAUNCH("csr_carry_kernel (runs)");
    hipLaunchKernelGGL(embed_heads_kernel<true>, dim3(hb), dim3(kHeadThreads), 0, st, keys, slots, sentinel, runs_cap, heads, run_row, runptr,
                       end_pos);
    SAGE_CHECK_LAUNCH("embed_heads_kernel (scatter)");
    hipLaunchKernelGGL(embed_runs_fill_kernel, dim3(sage_cdiv(runs_cap + 1, 256)), dim3(256), 0, st, (const int64_t*)heads, hb,
                       (const int64_t*)end_pos, runs_cap, runptr, num_rows_out);
    SAGE_CHECK_LAUNCH("embed_runs_fill_kernel");
    return SAGE_OK;
}

}  // namespace
