// Terms sorted by destination row, behind sage_embed_grad.hip and sage_csr_mean_backward_rows.hip: int32 (key, value) pairs with keys in
// [0, rows] (rows = the sentinel of an unused slot), a STABLE hipcub radix sort on the key bits that matter, so the order the terms
// were laid out in survives inside a run of equal keys, and over the sorted keys either a row pointer (one entry per row) or a run
// list (one entry per row that has a term: the _rows / _touched entries, which size nothing by `rows`).  The sort's temporary is reserved by
// host arithmetic (a workspace size query must answer without a device) and checked against the library before the sort.  What the sort
// and the run list need of a workspace (SortPairsWs, RunListWs) lives here too: the two files embed them in their layouts.
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

// Bytes reserved for the temporary of a sort of `slots` pairs.  The library's own size query asks the runtime for the device's
// architecture, so it answers only where there is a device; the layout has to be host arithmetic.  Reserved is a bound on what the
// sort partitions its temporary into: a second key and value array (8 bytes per slot), one look-back word per digit (256) and block
// of at least 512 slots (at most 4 bytes per slot at 8 bytes a word), digit histograms of a few KiB.  sort_temp_check asks the
// library before an entry launches anything and refuses (SAGE_ELAUNCH, nothing sorted) if it ever wanted more.
inline size_t sort_temp_reserve(int64_t slots) { return (size_t)slots * 16 + 65536; }

// What a sort of up to `slots` pairs needs of a workspace: the pairs as the caller's kernel lays them out (keys / vals), the sorted
// pairs, the library's temporary.
struct SortPairsWs {
    size_t keys_in, keys_out, vals_in, vals_out, cub, cub_bytes;
    void take(int64_t slots, WsCursor& cur) {
        for (size_t* field : {&keys_in, &keys_out, &vals_in, &vals_out}) *field = cur.take((size_t)slots * 4);
        cub_bytes = sort_temp_reserve(slots);
        cub = cur.take(cub_bytes);
    }
    int32_t* keys(void* ws) const { return (int32_t*)((char*)ws + keys_in); }
    int32_t* vals(void* ws) const { return (int32_t*)((char*)ws + vals_in); }
    int32_t* sorted_keys(void* ws) const { return (int32_t*)((char*)ws + keys_out); }
    int32_t* sorted_vals(void* ws) const { return (int32_t*)((char*)ws + vals_out); }
};

// Does the reserve hold the temporary of a sort of `slots` pairs?  Errors under the entry's `name`; called before the entry's first launch.
inline int sort_temp_check(const char* name, int slots, int bits, const SortPairsWs& S) {
    size_t sort_bytes = 0;
    if (hipcub::DeviceRadixSort::SortPairs(nullptr, sort_bytes, (const int32_t*)nullptr, (int32_t*)nullptr, (const int32_t*)nullptr,
                                           (int32_t*)nullptr, slots, 0, bits, (hipStream_t)0) != hipSuccess || sort_bytes > S.cub_bytes) {
        sage_set_error("%s: the radix sort asks for %zu bytes of temporary, %zu reserved", name, sort_bytes, S.cub_bytes);
        return SAGE_ELAUNCH;
    }
    return SAGE_OK;
}

// keys(ws) / vals(ws) -> sorted_keys(ws) / sorted_vals(ws), stable, on the low `bits` bits of the keys
inline int sort_pairs(const char* name, void* ws, const SortPairsWs& S, int slots, int bits, hipStream_t st) {
    size_t cub_bytes = S.cub_bytes;
    if (hipcub::DeviceRadixSort::SortPairs((char*)ws + S.cub, cub_bytes, (const int32_t*)S.keys(ws), S.sorted_keys(ws),
                                           (const int32_t*)S.vals(ws), S.sorted_vals(ws), slots, 0, bits, st) != hipSuccess) {
        sage_set_error("%s: radix sort failed", name);
        return SAGE_ELAUNCH;
    }
    return SAGE_OK;
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

inline int64_t run_head_blocks(int64_t slots) { return (slots + kHeadTile - 1) / kHeadTile; }

// What the run list of up to `slots` sorted keys with at most runs_cap runs needs of a workspace (heads: one entry per tile and one)
struct RunListWs {
    size_t run_row, runptr, heads, end_pos;
    int64_t runs_cap;
    void take(int64_t slots, int64_t cap, WsCursor& cur) {
        runs_cap = cap;
        run_row = cur.take((size_t)runs_cap * 4);
        runptr = cur.take((size_t)(runs_cap + 1) * 8);
        heads = cur.take((size_t)(run_head_blocks(slots) + 1) * 8);
        end_pos = cur.take(8);
    }
};

// The run list as the row passes read it: U = *num_runs, on the device
struct RunList { const int32_t* run_row; const int64_t* runptr; const int64_t* num_runs; };

// The run list of `slots` sorted keys (sentinel = rows; slots at most what W was taken for): count the heads per tile, scan the
// tiles, write the runs, close the list.  U is also stored to num_rows_out[0].
inline int sorted_run_list(const int32_t* keys, int slots, int sentinel, const RunListWs& W, void* workspace, int32_t* num_rows_out,
                           hipStream_t st, RunList* R) {
    char* ws = (char*)workspace;
    int32_t* run_row = (int32_t*)(ws + W.run_row);
    int64_t* runptr = (int64_t*)(ws + W.runptr);
    int64_t* heads = (int64_t*)(ws + W.heads);
    int64_t* end_pos = (int64_t*)(ws + W.end_pos);
    const int hb = (int)run_head_blocks(slots);
    hipLaunchKernelGGL(embed_heads_kernel<false>, dim3(hb), dim3(kHeadThreads), 0, st, keys, slots, sentinel, W.runs_cap, heads, run_row, runptr,
                       end_pos);
    SAGE_CHECK_LAUNCH("embed_heads_kernel (count)");
    hipLaunchKernelGGL(csr_carry_kernel, dim3(1), dim3(kCarryThreads), 0, st, heads, hb);
    SAGE_CHECK_LAUNCH("csr_carry_kernel (runs)");
    hipLaunchKernelGGL(embed_heads_kernel<true>, dim3(hb), dim3(kHeadThreads), 0, st, keys, slots, sentinel, W.runs_cap, heads, run_row, runptr,
                       end_pos);
    SAGE_CHECK_LAUNCH("embed_heads_kernel (scatter)");
    hipLaunchKernelGGL(embed_runs_fill_kernel, dim3(sage_cdiv(W.runs_cap + 1, 256)), dim3(256), 0, st, (const int64_t*)heads, hb,
                       (const int64_t*)end_pos, W.runs_cap, runptr, num_rows_out);
    SAGE_CHECK_LAUNCH("embed_runs_fill_kernel");
    *R = RunList{run_row, runptr, heads + hb};
    return SAGE_OK;
}

}  // namespace
