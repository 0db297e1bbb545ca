// The weighted term sum of the csr_mean adjoints: sage_csr_mean_backward.hip (whole graph, caller-built transpose, and its GROUPED
// form) and sage_csr_mean_backward_rows.hip (one seed batch, transpose sorted per call; every table row, or the touched rows only).  sum_weighted is the only place that forms a
// term -- ONE fma(w[x], grad_out[x], acc) -- and bwd_chunk_kernel / bwd_row_kernel hand it to sage_csr_common.h's chunked_row_sum, so
// every member of the family adds a row's terms in the same way and a row's bits depend on its term sequence alone.
// Internal linkage, as sage_csr_common.h: each translation unit that includes this holds its own copy of the kernels.
#pragma once
#include "sage_csr_common.h"

namespace {

// The largest r in [lo, hi] with rowptr[r] <= x (lo if there is none).  At most 32 steps whatever rowptr holds; r stays in [lo, hi].
__device__ inline int32_t row_of(const int64_t* __restrict__ rowptr, int32_t lo, int32_t hi, int64_t x) {
    for (int it = 0; it < 32 && lo < hi; ++it) {
        const int32_t mid = lo + (hi - lo + 1) / 2;
        if (rowptr[mid] <= x) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// acc = fma(w[x], grad_out[x], acc) over x = col_t[b..e) in stored order (the forward's sum_edges with a weight: ids AND weights
// broadcast by readlane, 8 rows in flight).  b, e wave-uniform.  Ids are clamped into [0, last_row].
template <int VEC>
__device__ inline void sum_weighted(const int32_t* __restrict__ col_t, int64_t b, int64_t e, const float* __restrict__ w,
                                    const float* __restrict__ g, int64_t ldg, int last_row, int c0, bool ok,
                                    typename VecT<VEC>::type& acc) {
    using V = typename VecT<VEC>::type;
    const int lane = sage_lane();
    for (int64_t base = b; base < e; base += kWave) {
        const int m = (int)min((int64_t)kWave, e - base);
        const int raw = (lane < m) ? col_t[base + lane] : 0;
        const int myid = min(max(raw, 0), last_row);     // never read outside grad_out / w
        const int mywt = (lane < m) ? __float_as_int(w[myid]) : 0;
        for (int j0 = 0; j0 < m; j0 += 8) {
            V t[8];
            float wt[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int j = min(j0 + u, m - 1);
                const int id = __builtin_amdgcn_readlane(myid, j);
                wt[u] = __int_as_float(__builtin_amdgcn_readlane(mywt, j));
                if (ok) t[u] = *reinterpret_cast<const V*>(g + (int64_t)id * ldg + c0);
                else vfill(t[u], 0.f);
            }
#pragma unroll
            for (int u = 0; u < 8; ++u)
                if (j0 + u < m) vfma(acc, wt[u], t[u]);
        }
    }
}

// 4. one wave per item (row, chunk): partials[item] := the chunk's weighted sum
template <int VEC, bool GROUPED>
__global__ __launch_bounds__(256) void bwd_chunk_kernel(const int64_t* __restrict__ rowptr_t, const int32_t* __restrict__ col_t,
                                                        int64_t num_nodes, const int32_t* __restrict__ nodes, int n,
                                                        const float* __restrict__ w, const float* __restrict__ g, int64_t ldg, int dim,
                                                        const int64_t* __restrict__ off, const int64_t* __restrict__ carry, int nb,
                                                        int64_t cap, const int32_t* __restrict__ item_row, float* __restrict__ partials,
                                                        int64_t num_src) {
    using V = typename VecT<VEC>::type;
    const int lane = sage_lane();
    const int64_t wave = (int64_t)((blockIdx.x * blockDim.x + threadIdx.x) >> 6);
    const int64_t nwaves = (int64_t)((gridDim.x * blockDim.x) >> 6);
    const int64_t items = min(carry[nb], cap);
    const int64_t total = rowptr_t[num_nodes];
    const int last_row = (int)(GROUPED ? num_src : num_nodes) - 1;      // GROUPED: num_nodes counts the rows (groups), num_src the sources
    for (int64_t i = wave; i < items; i += nwaves) {
        int32_t v;
        int64_t cb, ce;
        if (!chunk_item<true>(i, item_row, rowptr_t, num_nodes, nodes, n, total, off, cap, v, cb, ce)) continue;
        for (int cbk = 0; cbk < dim; cbk += kWave * VEC) {
            const int c0 = cbk + lane * VEC;
            const bool ok = c0 < dim;
            V acc;
            vfill(acc, 0.f);
            sum_weighted<VEC>(col_t, cb, ce, w, g, ldg, last_row, c0, ok, acc);
            if (ok) *reinterpret_cast<V*>(partials + i * dim + c0) = acc;
        }
    }
}

// 5. one wave per row of grad_table
template <int VEC, bool GROUPED>
__global__ __launch_bounds__(256) void bwd_row_kernel(const int64_t* __restrict__ rowptr_t, const int32_t* __restrict__ col_t,
                                                      int64_t num_nodes, const int32_t* __restrict__ nodes, int n,
                                                      const float* __restrict__ w, const int32_t* __restrict__ flag,
                                                      const float* __restrict__ g, int64_t ldg, int dim,
                                                      const int64_t* __restrict__ off, int64_t cap, const float* __restrict__ partials,
                                                      float* __restrict__ grad_table, int64_t ldgt, int64_t num_src) {
    using V = typename VecT<VEC>::type;
    const int lane = sage_lane();
    const int wave = (int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6);
    const int nwaves = (int)((gridDim.x * blockDim.x) >> 6);
    const int last_row = (int)(GROUPED ? num_src : num_nodes) - 1;      // as in bwd_chunk_kernel
    const int64_t total = rowptr_t[num_nodes];
    for (int r = wave; r < n; r += nwaves) {
        int32_t u;
        int64_t b, e;
        row_span<true>(rowptr_t, num_nodes, nodes, r, total, u, b, e);
        const int64_t k = long_chunks(e - b);
        const int64_t o = first_item<true>(off, r, k);
        const bool extra = !GROUPED && u >= 0 && __builtin_amdgcn_readfirstlane(flag[max(u, 0)]) != 0;   // GROUPED: the list holds the self entries
        const float wu = extra ? __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(w[u]))) : 0.f;
        for (int cb = 0; cb < dim; cb += kWave * VEC) {
            const int c0 = cb + lane * VEC;
            const bool ok = c0 < dim;
            V s = chunked_row_sum<V>(k, o, cap, partials, dim, c0, ok, b, e, [&](int64_t tb, int64_t te, V& acc) {
                sum_weighted<VEC>(col_t, tb, te, w, g, ldg, last_row, c0, ok, acc);
            });
            if (ok) {
                if (extra) vfma(s, wu, *reinterpret_cast<const V*>(g + (int64_t)u * ldg + c0));   // the self term, last
                *reinterpret_cast<V*>(grad_table + (int64_t)r * ldgt + c0) = s;
            }
        }
    }
}

// 5'. one wave per RUN u < U of a run list (sage_sorted_terms.h; U read on the device), GROUPED: the run's sum -- bwd_row_kernel's, the
// same chunked_row_sum over the same sum_weighted -- stored as row u of the compact gradient (u < max_rows) and / or applied to row
// run_row[u] of the table: table = fma(-lr, sum, table), one rounding.  Rows without a run are neither read nor written.
template <int VEC>
__global__ __launch_bounds__(256) void bwd_runs_row_kernel(const int64_t* __restrict__ runptr, const int32_t* __restrict__ col_t, int runs_cap,
                                                           const int64_t* __restrict__ num_runs, const float* __restrict__ w,
                                                           const float* __restrict__ g, int64_t ldg, int dim, const int64_t* __restrict__ off,
                                                           int64_t cap, const float* __restrict__ partials, int64_t num_src,
                                                           const int32_t* __restrict__ run_row, int32_t* __restrict__ rows_out,
                                                           float* __restrict__ grad_rows, int64_t max_rows, int64_t ldr,
                                                           float* __restrict__ table, int64_t ldt, int num_rows, float lr) {
    using V = typename VecT<VEC>::type;
    const int lane = sage_lane();
    const int wave = (int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6);
    const int nwaves = (int)((gridDim.x * blockDim.x) >> 6);
    const int last_row = (int)num_src - 1;
    const int64_t total = runptr[runs_cap];
    const int nruns = (int)min(uniform64(*num_runs), (int64_t)runs_cap);
    for (int u = wave; u < nruns; u += nwaves) {
        int32_t v;
        int64_t b, e;
        row_span<true>(runptr, runs_cap, nullptr, u, total, v, b, e);
        const int64_t k = long_chunks(e - b);
        const int64_t o = first_item<true>(off, u, k);
        const int row = min(max(__builtin_amdgcn_readfirstlane(run_row[u]), 0), num_rows - 1);   // a key of the layout: inside the table already
        const bool keep = grad_rows != nullptr && u < max_rows;
        if (keep && lane == 0) rows_out[u] = row;
        for (int cb = 0; cb < dim; cb += kWave * VEC) {
            const int c0 = cb + lane * VEC;
            const bool ok = c0 < dim;
            const V s = chunked_row_sum<V>(k, o, cap, partials, dim, c0, ok, b, e, [&](int64_t tb, int64_t te, V& acc) {
                sum_weighted<VEC>(col_t, tb, te, w, g, ldg, last_row, c0, ok, acc);
            });
            if (ok) {
                if (keep) *reinterpret_cast<V*>(grad_rows + (int64_t)u * ldr + c0) = s;
                if (table) {
                    V* p = reinterpret_cast<V*>(table + (int64_t)row * ldt + c0);
                    V x = *p;
                    vfma(x, -lr, s);
                    *p = x;
                }
            }
        }
    }
}

// What the two passes sum: the n rows (`nodes`, or row r itself) of the CSR (rowptr_t, col_t) over num_rows rows, whose entries name
// rows of w and grad_out.  grouped: w and grad_out have num_src rows and the list holds the self entries (flag is not read).
struct BwdSum {
    const int64_t* rowptr_t; const int32_t* col_t; int64_t num_rows; bool grouped;
    const int32_t* nodes; int32_t n;
    const float* w; const int32_t* flag; int64_t num_src;
    const float* grad_out; int64_t ldg; int32_t dim;
    float* grad_table; int64_t ldgt;
};

// Launches 1-4 of the family: the chunk plan over the rows and the chunk pass.  vec4: 16-byte accesses (the caller's outputs included).
inline int bwd_chunk_launch(const BwdSum& s, bool vec4, void* workspace, const ChunkWs& C, hipStream_t st, ChunkPlan* plan) {
    if (const int rc = csr_chunk_plan(s.rowptr_t, s.num_rows, s.nodes, s.n, workspace, C, st, plan)) return rc;
    const ChunkPlan& P = *plan;
    if (P.cap > 0) {
        const int blocks = (int)std::min<int64_t>((P.cap + 3) / 4, kNumCU * 8);
#define SAGE_BWD_CHUNK(VEC, GROUPED)                                                                                                    \
    hipLaunchKernelGGL((bwd_chunk_kernel<VEC, GROUPED>), dim3(blocks), dim3(256), 0, st, s.rowptr_t, s.col_t, s.num_rows, s.nodes, s.n, s.w, \
                       s.grad_out, s.ldg, s.dim, P.off, P.carry, P.nb, P.cap, P.item_row, P.partials, s.num_src)
        if (s.grouped) { if (vec4) SAGE_BWD_CHUNK(4, true); else SAGE_BWD_CHUNK(1, true); }
        else { if (vec4) SAGE_BWD_CHUNK(4, false); else SAGE_BWD_CHUNK(1, false); }
#undef SAGE_BWD_CHUNK
        SAGE_CHECK_LAUNCH("bwd_chunk_kernel");
    }
    return SAGE_OK;
}

// Launches 1-5 of the family: the chunk plan over the rows, the chunk pass, the row pass.
inline int bwd_sum_launch(const BwdSum& s, void* workspace, const ChunkWs& C, hipStream_t st) {
    const bool vec4 = (s.dim % 4 == 0) && (s.ldg % 4 == 0) && (s.ldgt % 4 == 0) && sage_aligned(s.grad_out, 16) && sage_aligned(s.grad_table, 16);
    ChunkPlan P;
    if (const int rc = bwd_chunk_launch(s, vec4, workspace, C, st, &P)) return rc;
    const int blocks = std::min(sage_cdiv(s.n, 4), kNumCU * 8);
#define SAGE_BWD_ROW(VEC, GROUPED)                                                                                                        \
    hipLaunchKernelGGL((bwd_row_kernel<VEC, GROUPED>), dim3(blocks), dim3(256), 0, st, s.rowptr_t, s.col_t, s.num_rows, s.nodes, s.n, s.w, s.flag, \
                       s.grad_out, s.ldg, s.dim, P.off, P.cap, P.partials, s.grad_table, s.ldgt, s.num_src)
    if (s.grouped) { if (vec4) SAGE_BWD_ROW(4, true); else SAGE_BWD_ROW(1, true); }
    else { if (vec4) SAGE_BWD_ROW(4, false); else SAGE_BWD_ROW(1, false); }
#undef SAGE_BWD_ROW
    SAGE_CHECK_LAUNCH("bwd_row_kernel");
    return SAGE_OK;
}

}  // namespace
