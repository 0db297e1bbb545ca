// The chunked row sum behind sage_csr_mean.hip, sage_csr_sum.hip, sage_csr_mean_backward.hip and sage_embed_grad.hip: rows longer
// than SAGE_CSR_MEAN_CHUNK entries are cut into chunks, every chunk is summed in stored order, a row's partials are added in chunk
// order, no float atomics.  This header holds the ONE copy of that rule:
//   host    WsCursor / ChunkWs / chunk_ws (the workspace sub-layout), csr_chunk_plan (launches 1-3: count -> carry -> expand; see
//           the head of sage_csr_mean.hip), csr_workspace_check
//   device  row_span (the clamped row), chunk_item (is item i a chunk of a row that fits, and which entries), chunked_row_sum (a
//           row's total: its partials, its entries in place, or -- a long row without workspace room -- the chunk pass's sums
//           redone with the same operations in the same order), sum_edges (the unweighted term walker)
// What differs per file is the TERM (a table row, a weighted gradient row) and what happens to a row's total; each file hands its
// term walker to chunked_row_sum, so "same bits in the chunk pass and in the fall-back" holds by construction.
// Everything has internal linkage: each translation unit that includes this holds its own copy of the kernels.
#pragma once
#include "sage_internal.h"

#include <algorithm>
#include <type_traits>

namespace {

constexpr int64_t kChunk = SAGE_CSR_MEAN_CHUNK;
constexpr int kCountThreads = 256, kCountIpt = 8, kCountTile = kCountThreads * kCountIpt;
constexpr int kCarryThreads = 1024;

size_t align256(size_t x) { return (x + 255) / 256 * 256; }

// Eight columns of a lane: two float4, stored and loaded as such (the bf16 table's 16-byte form, see load_cols).
struct alignas(16) float8 { float4 lo, hi; };

template <int VEC> struct VecT;
template <> struct VecT<8> { using type = float8; };
template <> struct VecT<4> { using type = float4; };
template <> struct VecT<1> { using type = float; };

__device__ inline void vadd(float4& a, const float4& b) { a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w; }
__device__ inline void vadd(float& a, const float& b) { a += b; }
__device__ inline float4 vscale(const float4& a, float s) { return make_float4(a.x * s, a.y * s, a.z * s, a.w * s); }
__device__ inline float vscale(const float& a, float s) { return a * s; }
__device__ inline void vfill(float4& a, float s) { a = make_float4(s, s, s, s); }
__device__ inline void vfill(float& a, float s) { a = s; }
__device__ inline void vfma(float4& a, float s, const float4& b) {
    a.x = __builtin_fmaf(s, b.x, a.x); a.y = __builtin_fmaf(s, b.y, a.y); a.z = __builtin_fmaf(s, b.z, a.z); a.w = __builtin_fmaf(s, b.w, a.w);
}
__device__ inline void vfma(float& a, float s, const float& b) { a = __builtin_fmaf(s, b, a); }
__device__ inline void vadd(float8& a, const float8& b) { vadd(a.lo, b.lo); vadd(a.hi, b.hi); }
__device__ inline float8 vscale(const float8& a, float s) { return float8{vscale(a.lo, s), vscale(a.hi, s)}; }
__device__ inline void vfill(float8& a, float s) { vfill(a.lo, s); vfill(a.hi, s); }

__device__ inline int64_t uniform64(int64_t x) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)x);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)((uint64_t)x >> 32));
    return (int64_t)(((uint64_t)hi << 32) | lo);
}

// UNIFORM: the caller is ONE WAVE per row or item, so what it reads about the row is the same in every lane and is broadcast from the
// first lane (it then lives in scalar registers).  The lane-group kernels of sage_embed_grad.hip hold several rows in a wave: they
// pass false and every lane keeps its own value.  A template parameter, so that no caller can forget which it is.
template <bool UNIFORM> __device__ inline int32_t bcast(int32_t x) {
    if constexpr (UNIFORM) return __builtin_amdgcn_readfirstlane(x);
    else return x;
}
template <bool UNIFORM> __device__ inline int64_t bcast(int64_t x) {
    if constexpr (UNIFORM) return uniform64(x);
    else return x;
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

template <bool UNIFORM>
__device__ inline void row_span(const int64_t* __restrict__ rowptr, int64_t num_nodes, const int32_t* __restrict__ nodes, int r,
                                int64_t total, int32_t& v, int64_t& b, int64_t& e) {
    row_span(rowptr, num_nodes, nodes, r, total, v, b, e);
    v = bcast<UNIFORM>(v);
    b = bcast<UNIFORM>(b);
    e = bcast<UNIFORM>(e);
}

__device__ inline int64_t long_chunks(int64_t deg) { return deg > kChunk ? (deg + kChunk - 1) / kChunk : 0; }

// Did the chunk pass sum the k chunks of the row whose first item is o?  (k == 0: a row of one chunk, which has no items.)
__device__ inline bool chunks_fit(int64_t k, int64_t o, int64_t cap) { return k > 0 && o + k <= cap; }

// The first item of row r, read only where the row has items.
template <bool UNIFORM> __device__ inline int64_t first_item(const int64_t* __restrict__ off, int64_t r, int64_t k) {
    return k > 0 ? bcast<UNIFORM>(off[r]) : 0;
}

// The block scan of a count kernel (kCountThreads threads): every thread holds the counts c[] of kCountIpt consecutive rows from row
// r0 on (0 at or past n); off[r] := block-local exclusive offset, carry[block] := the block's sum.  Within the wave by shuffles,
// then across the 4 waves.
__device__ inline void count_block_scan(const int64_t (&c)[kCountIpt], int r0, int n, int64_t* __restrict__ off, int64_t* __restrict__ carry) {
    __shared__ int64_t wave_sum[kCountThreads / kWave];
    int64_t s = 0;
#pragma unroll
    for (int i = 0; i < kCountIpt; ++i) s += c[i];
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

// 1. per-thread kCountIpt consecutive rows; off[r] := block-local exclusive offset, carry[block] := the block's chunk sum
__global__ __launch_bounds__(kCountThreads) void csr_count_kernel(const int64_t* __restrict__ rowptr, int64_t num_nodes,
                                                                   const int32_t* __restrict__ nodes, int n, int64_t* __restrict__ off,
                                                                   int64_t* __restrict__ carry) {
    const int64_t total = rowptr[num_nodes];
    const int r0 = blockIdx.x * kCountTile + threadIdx.x * kCountIpt;
    int64_t c[kCountIpt];
#pragma unroll
    for (int i = 0; i < kCountIpt; ++i) {
        c[i] = 0;
        if (r0 + i < n) {
            int32_t v;
            int64_t b, e;
            row_span(rowptr, num_nodes, nodes, r0 + i, total, v, b, e);
            c[i] = long_chunks(e - b);
        }
    }
    count_block_scan(c, r0, n, off, carry);
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
    if (chunks_fit(k, o, cap))
        for (int64_t c = 0; c < k; ++c) item_row[o + c] = r;
}

// Item i of the chunk pass: false if it is no chunk of a row that fits, else v = the row's node (-1: none) and [cb, ce) = the chunk's
// entries.  With a max_edges below the truth the entries of a row that did not fit were never written: an entry counts only if it
// names a row whose chunk range fits and holds i (the ranges are disjoint, so a stale value cannot pass).  Nothing is read through an
// entry that names no row.  One exit on purpose: with a return per refusal hipcc schedules embed_chunk_kernel's walk so that a trip
// waits for all of its rows before the first fma (measured: sage_embed_grad 252 us against 245).
template <bool UNIFORM>
__device__ inline bool chunk_item(int64_t i, const int32_t* __restrict__ item_row, const int64_t* __restrict__ rowptr, int64_t num_nodes,
                                  const int32_t* __restrict__ nodes, int n, int64_t total, const int64_t* __restrict__ off, int64_t cap,
                                  int32_t& v, int64_t& cb, int64_t& ce) {
    const int r = bcast<UNIFORM>(item_row[i]);
    bool mine = r >= 0 && r < n;
    int64_t b = 0, e = 0, o = 0;
    v = -1;
    if (mine) {
        row_span<UNIFORM>(rowptr, num_nodes, nodes, r, total, v, b, e);
        const int64_t k = long_chunks(e - b);
        o = bcast<UNIFORM>(off[r]);
        mine = !(k == 0 || o + k > cap || i < o || i >= o + k);
    }
    cb = b + (i - o) * kChunk;
    ce = min(cb + kChunk, e);
    return mine;
}

// THE arithmetic of a row, the only copy of it: lane columns [c0, c0 + width of V) of the total of row [b, e), whose k chunks start
// at item o.  term(b, e, acc) is the file's walker: acc += the terms of entries [b, e) in stored order.  ok: the lane holds columns.
template <typename V, typename Term>
__device__ inline V chunked_row_sum(int64_t k, int64_t o, int64_t cap, const float* __restrict__ partials, int dim, int c0, bool ok,
                                    int64_t b, int64_t e, Term term) {
    V s;
    vfill(s, 0.f);
    if (chunks_fit(k, o, cap)) {                      // the chunk pass summed this row's chunks
        if (ok)
            for (int64_t c = 0; c < k; ++c) vadd(s, *reinterpret_cast<const V*>(partials + (o + c) * dim + c0));
    } else if (__builtin_expect(k == 0, 1)) {         // nearly every row, so the straight path: as a taken branch to the end of the
                                                      // kernel it cost sage_csr_sum, whose groups are mostly empty, 2 % (0.349 ms for 0.342)
        term(b, e, s);
    } else {                                          // long row without workspace room: the chunk pass's sums, here
        for (int64_t c = 0; c < k; ++c) {
            V p;
            vfill(p, 0.f);
            term(b + c * kChunk, min(b + (c + 1) * kChunk, e), p);
            vadd(s, p);
        }
    }
    return s;
}

// The table's element type TT: float, or uint16_t = a bf16 value as its raw 16 bits (sage_csr_mean_bf16).  A bf16 value widens to
// fp32 EXACTLY (bits << 16), so everything after the load is the fp32 arithmetic on the widened table, bit for bit.  On the vector path
// a lane keeps its four columns [c0, c0 + 4): a float table gives them as one 16-byte load, a bf16 table as one 8-byte load whose two
// words each hold two columns, the lower column in the low half (little endian).
// A load and its widening are two steps, so that a trip's loads are all issued before the first of them is waited for: what is
// in flight is the RAW value (the 8 bytes), widened only where it is added.
template <typename V, typename TT> struct RawT { using type = V; };                       // a float table: the columns themselves
template <> struct RawT<float8, uint16_t> { using type = uint4; };
template <> struct RawT<float4, uint16_t> { using type = uint2; };
template <> struct RawT<float, uint16_t> { using type = uint32_t; };

template <typename V, typename TT> __device__ inline typename RawT<V, TT>::type load_raw(const TT* __restrict__ p) {
    if constexpr (std::is_same_v<TT, float>) return *reinterpret_cast<const V*>(p);
    else if constexpr (std::is_same_v<V, float>) return (uint32_t)*p;
    else return *reinterpret_cast<const typename RawT<V, TT>::type*>(p);
}
__device__ inline void zero_raw(float8& a) { vfill(a, 0.f); }
__device__ inline void zero_raw(float4& a) { vfill(a, 0.f); }
__device__ inline void zero_raw(float& a) { vfill(a, 0.f); }
__device__ inline void zero_raw(uint4& a) { a = make_uint4(0, 0, 0, 0); }
__device__ inline void zero_raw(uint2& a) { a = make_uint2(0, 0); }
__device__ inline void zero_raw(uint32_t& a) { a = 0; }

__device__ inline float4 widen2(uint32_t x, uint32_t y) {
    return make_float4(__uint_as_float(x << 16), __uint_as_float(x & 0xffff0000u), __uint_as_float(y << 16), __uint_as_float(y & 0xffff0000u));
}
template <typename V> __device__ inline V widen(const V& raw) { return raw; }
template <typename V> __device__ inline V widen(const uint4& w) { return float8{widen2(w.x, w.y), widen2(w.z, w.w)}; }
template <typename V> __device__ inline V widen(const uint2& w) { return widen2(w.x, w.y); }
template <typename V> __device__ inline V widen(const uint32_t& w) { return __uint_as_float(w << 16); }

template <typename V, typename TT> __device__ inline V load_cols(const TT* __restrict__ p) { return widen<V>(load_raw<V>(p)); }

// Rows of a trip whose loads are in flight together before the first add.  A bf16 row is half the bytes; measured (DESIGN.md section
// 9a, configs[2]'s graph, width 256): 8 rows 6.00 ms, 16 rows 5.53, 32 rows 5.34, against 9.76 for the float table's 8 x 16 bytes.
// The depth never changes the order of a column's additions.
#ifndef SAGE_CSR_BF16_IN_FLIGHT
#define SAGE_CSR_BF16_IN_FLIGHT 32
#endif
template <typename TT> struct InFlight { static constexpr int rows = 8; };
template <> struct InFlight<uint16_t> { static constexpr int rows = SAGE_CSR_BF16_IN_FLIGHT; };
static_assert(kWave % InFlight<uint16_t>::rows == 0, "a wave trip is a whole number of in-flight groups");

// acc += table rows of col[b..e) in stored order (the sage_gather.hip inner loop: ids broadcast by readlane, 8 rows in flight).
// b, e wave-uniform.  SELF: found |= some entry of the range is node v (compiled out otherwise: v and found are not touched).
// IDX: the id is a node id, clamped into [0, last_node]; the row read is index[id], clamped into [0, last_row].
template <int VEC, bool IDX, bool SELF, typename TT>
__device__ inline void sum_edges(const int32_t* __restrict__ col, int64_t b, int64_t e, const TT* __restrict__ table, int64_t ld,
                                 int last_row, int c0, bool ok, int32_t v, typename VecT<VEC>::type& acc, bool& found,
                                 const int32_t* __restrict__ index, int last_node) {
    using V = typename VecT<VEC>::type;
    constexpr int kRows = InFlight<TT>::rows;
    const int lane = sage_lane();
    for (int64_t base = b; base < e; base += kWave) {
        const int m = (int)min((int64_t)kWave, e - base);
        const int raw = (lane < m) ? col[base + lane] : -1;
        if constexpr (SELF)
            if (__any(lane < m && raw == v)) found = true;
        int myid;
        if constexpr (IDX) {
            const int node = min(max(raw, 0), last_node);                            // never read outside index[]
            myid = min(max(lane < m ? index[node] : 0, 0), last_row);                // ... nor outside embed[]
        } else {
            myid = min(max(raw, 0), last_row);           // never read outside the table
        }
        for (int j0 = 0; j0 < m; j0 += kRows) {
            typename RawT<V, TT>::type t[kRows];
#pragma unroll
            for (int u = 0; u < kRows; ++u) {
                const int id = __builtin_amdgcn_readlane(myid, min(j0 + u, m - 1));
                if (ok) t[u] = load_raw<V>(table + (int64_t)id * ld + c0);
                else zero_raw(t[u]);
            }
#pragma unroll
            for (int u = 0; u < kRows; ++u)
                if (j0 + u < m) vadd(acc, widen<V>(t[u]));
        }
    }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------
// A workspace is cut front to back into 256-byte aligned pieces; every take aligns on its own, so a layout's total does not depend on
// the order of its fields.
struct WsCursor {
    size_t off = 0;
    size_t take(size_t bytes) {
        const size_t o = off;
        off = align256(off + std::max<size_t>(bytes, 1));
        return o;
    }
};

// What the chunk split of `rows` rows needs of a workspace; every file's layout holds one beside its own fields.
struct ChunkWs {
    size_t off, carry, item_row, partials;
    int64_t cap;       // item entries (= partial rows) the workspace holds
    int64_t nblocks;   // count-kernel blocks
};

// Item entries a workspace sized for max_edges holds: the chunks of all long rows are at most floor(E_sel / E) + (number of long
// rows), and a long row has more than E edges.  false: more than an int32 item index reaches.  rows, max_edges >= 0.
// tests/test_gpu_csr_plan.py reads the first two pieces back, in this order: off[rows], then carry[nblocks + 1] (sage_csr_mean's workspace).
inline bool chunk_ws(int64_t rows, int64_t max_edges, int32_t dim, WsCursor& cur, ChunkWs* C) {
    C->cap = max_edges / kChunk + std::min<int64_t>(rows, max_edges / (kChunk + 1));
    if (C->cap >= (1ll << 31)) return false;
    C->nblocks = (rows + kCountTile - 1) / kCountTile;
    C->off = cur.take((size_t)rows * 8);
    C->carry = cur.take((size_t)(C->nblocks + 1) * 8);
    C->item_row = cur.take((size_t)C->cap * 4);
    C->partials = cur.take((size_t)C->cap * (size_t)dim * 4);
    return true;
}

// The arrays of a ChunkWs inside a workspace, as the chunk and row kernels take them.
struct ChunkPlan {
    int64_t* off;
    int64_t* carry;
    int32_t* item_row;
    float* partials;
    int64_t cap;
    int nb;
};

// Launches 1-3 over the n rows of (rowptr, nodes): afterwards off[r] is row r's first item, carry[nb] the number of items, and the
// items that fit name their rows.
inline int csr_chunk_plan(const int64_t* rowptr, int64_t num_nodes, const int32_t* nodes, int n, void* workspace, const ChunkWs& C,
                          hipStream_t st, ChunkPlan* P) {
    char* ws = (char*)workspace;
    *P = ChunkPlan{(int64_t*)(ws + C.off), (int64_t*)(ws + C.carry), (int32_t*)(ws + C.item_row), (float*)(ws + C.partials), C.cap, (int)C.nblocks};
    hipLaunchKernelGGL(csr_count_kernel, dim3(P->nb), dim3(kCountThreads), 0, st, rowptr, num_nodes, nodes, n, P->off, P->carry);
    SAGE_CHECK_LAUNCH("csr_count_kernel");
    hipLaunchKernelGGL(csr_carry_kernel, dim3(1), dim3(kCarryThreads), 0, st, P->carry, P->nb);
    SAGE_CHECK_LAUNCH("csr_carry_kernel");
    hipLaunchKernelGGL(csr_expand_kernel, dim3(sage_cdiv(n, 256)), dim3(256), 0, st, rowptr, num_nodes, nodes, n, P->off, (const int64_t*)P->carry,
                       C.cap, P->item_row);
    SAGE_CHECK_LAUNCH("csr_expand_kernel");
    return SAGE_OK;
}

// The last refusals of every entry: a workspace too small (or none), then one that is not aligned.
inline int csr_workspace_check(const char* name, const void* workspace, size_t workspace_bytes, size_t need) {
    if (workspace_bytes < need || !workspace) {
        sage_set_error("%s: workspace of %zu bytes, %zu needed", name, workspace_bytes, need);
        return SAGE_ENOSPACE;
    }
    SAGE_REQUIRE(sage_aligned(workspace, 256), "%s: workspace not 256-byte aligned", name);
    return SAGE_OK;
}

}  // namespace
