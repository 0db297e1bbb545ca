// csr_sum: per-row SUM of table rows over a rectangular CSR (num_rows groups over table_rows source rows) -- the reduction
// behind the gradient of a shared embedding row (aggregators.py:68-71: every node of one index reads one row of `embed`):
//     grad_embed[k] = sum over the nodes v with index[v] = k of grad_X[v]
// The grouping (rowptr, col) is built once per graph (ops.group_rows).  Its row lengths are the histogram of the index -- for
// node_degree the degree histogram of a power-law graph: a few rows hold most of the nodes, most rows are empty -- so this is
// sage_csr_mean's split (sage_csr_mean.hip) without its division, self term and NaN rule:
//   1-3. count, carry, expand (sage_csr_common.h)
//   4. chunk   one wave per item: partials[item] := the sum of the chunk's SAGE_CSR_MEAN_CHUNK entries
//   5. rows    one wave per row: short rows summed in place; long rows = their partials in chunk order; store
// A long row whose chunks do not fit the workspace is summed chunk by chunk by its row wave, with the same operations in the
// same order.  No float atomics; every row of out is stored, an empty row as zeros.
//
// Arithmetic of a row (its bits depend on nothing else): p_c = 0 + t_0 + t_1 + ... over chunk c's entries in stored order;
// out[r] = 0 + p_0 + p_1 + ... for a row of more than one chunk, out[r] = p_0 for any other.
#include "sage_csr_common.h"

namespace {

struct SumLayout {
    size_t off, carry, item_row, partials, total;
    int64_t cap;       // item entries (= partial rows) the workspace holds
    int64_t nblocks;   // count-kernel blocks
};

bool sum_layout(int64_t num_rows, int64_t max_edges, int32_t dim, SumLayout* L) {
    if (num_rows < 0 || num_rows >= (1ll << 31) || max_edges < 0 || dim < 1) return false;
    L->cap = csr_item_cap((int32_t)num_rows, max_edges);
    if (L->cap >= (1ll << 31)) return false;
    L->nblocks = (num_rows + kCountTile - 1) / kCountTile;
    size_t off = 0;
    auto take = [&](size_t bytes) { size_t o = off; off = align256(off + std::max<size_t>(bytes, 1)); return o; };
    L->off = take((size_t)num_rows * 8);
    L->carry = take((size_t)(L->nblocks + 1) * 8);
    L->item_row = take((size_t)L->cap * 4);
    L->partials = take((size_t)L->cap * (size_t)dim * 4);
    L->total = off;
    return true;
}

// acc += table rows of col[b..e) in stored order (the sage_csr_mean.hip inner loop: ids broadcast by readlane, 8 rows in flight).
// b, e wave-uniform.  Ids are clamped into the table.
template <int VEC>
__device__ inline void sum_rows(const int32_t* __restrict__ col, int64_t b, int64_t e, const float* __restrict__ table, int64_t ld,
                                int last_row, int c0, bool ok, typename VecT<VEC>::type& acc) {
    using V = typename VecT<VEC>::type;
    const int lane = sage_lane();
    for (int64_t base = b; base < e; base += kWave) {
        const int m = (int)min((int64_t)kWave, e - base);
        const int raw = (lane < m) ? col[base + lane] : 0;
        const int myid = min(max(raw, 0), last_row);     // never read outside the table
        for (int j0 = 0; j0 < m; j0 += 8) {
            V t[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int id = __builtin_amdgcn_readlane(myid, min(j0 + u, m - 1));
                if (ok) t[u] = *reinterpret_cast<const V*>(table + (int64_t)id * ld + c0);
                else vfill(t[u], 0.f);
            }
#pragma unroll
            for (int u = 0; u < 8; ++u)
                if (j0 + u < m) vadd(acc, t[u]);
        }
    }
}

// 4. one wave per item (row, chunk): partials[item] := the chunk's sum
template <int VEC>
__global__ __launch_bounds__(256) void sum_chunk_kernel(const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col, int64_t num_rows,
                                                        const float* __restrict__ table, int table_rows, int64_t ld, int dim,
                                                        const int64_t* __restrict__ off, const int64_t* __restrict__ carry, int nb,
                                                        int64_t cap, const int32_t* __restrict__ item_row, float* __restrict__ partials) {
    using V = typename VecT<VEC>::type;
    const int lane = sage_lane();
    const int n = (int)num_rows;
    const int64_t wave = (int64_t)((blockIdx.x * blockDim.x + threadIdx.x) >> 6);
    const int64_t nwaves = (int64_t)((gridDim.x * blockDim.x) >> 6);
    const int64_t items = min(carry[nb], cap);
    const int64_t total = rowptr[num_rows];
    for (int64_t i = wave; i < items; i += nwaves) {
        // an entry of a row that did not fit was never written: take one only if it names a row whose chunk range fits and holds i
        const int r = __builtin_amdgcn_readfirstlane(item_row[i]);
        if (r < 0 || r >= n) continue;
        int32_t v;
        int64_t b, e;
        row_span(rowptr, num_rows, nullptr, r, total, v, b, e);
        b = uniform64(b);
        e = uniform64(e);
        const int64_t k = long_chunks(e - b), o = uniform64(off[r]);
        if (k == 0 || o + k > cap || i < o || i >= o + k) continue;
        const int64_t cb = b + (i - o) * kChunk;
        const int64_t ce = min(cb + kChunk, e);
        for (int cbk = 0; cbk < dim; cbk += kWave * VEC) {
            const int c0 = cbk + lane * VEC;
            const bool ok = c0 < dim;
            V acc;
            vfill(acc, 0.f);
            sum_rows<VEC>(col, cb, ce, table, ld, table_rows - 1, c0, ok, acc);
            if (ok) *reinterpret_cast<V*>(partials + i * dim + c0) = acc;
        }
    }
}

// 5. one wave per row
template <int VEC>
__global__ __launch_bounds__(256) void sum_row_kernel(const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col, int64_t num_rows,
                                                      const float* __restrict__ table, int table_rows, int64_t ld, int dim,
                                                      const int64_t* __restrict__ off, int64_t cap, const float* __restrict__ partials,
                                                      float* __restrict__ out, int64_t ldo) {
    using V = typename VecT<VEC>::type;
    const int lane = sage_lane();
    const int n = (int)num_rows;
    const int wave = (int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6);
    const int nwaves = (int)((gridDim.x * blockDim.x) >> 6);
    const int last_row = table_rows - 1;
    const int64_t total = rowptr[num_rows];
    for (int r = wave; r < n; r += nwaves) {
        int32_t v;
        int64_t b, e;
        row_span(rowptr, num_rows, nullptr, r, total, v, b, e);
        b = uniform64(b);
        e = uniform64(e);
        const int64_t k = long_chunks(e - b);
        const int64_t o = k > 0 ? uniform64(off[r]) : 0;
        const bool split = k > 0 && o + k <= cap;        // the chunk pass summed this row's chunks
        for (int cb = 0; cb < dim; cb += kWave * VEC) {
            const int c0 = cb + lane * VEC;
            const bool ok = c0 < dim;
            V s;
            vfill(s, 0.f);
            if (split) {
                if (ok)
                    for (int64_t c = 0; c < k; ++c) vadd(s, *reinterpret_cast<const V*>(partials + (o + c) * dim + c0));
            } else if (k == 0) {
                sum_rows<VEC>(col, b, e, table, ld, last_row, c0, ok, s);
            } else {                                      // long row without workspace room: the chunk pass's sums, here
                for (int64_t c = 0; c < k; ++c) {
                    V p;
                    vfill(p, 0.f);
                    sum_rows<VEC>(col, b + c * kChunk, min(b + (c + 1) * kChunk, e), table, ld, last_row, c0, ok, p);
                    vadd(s, p);
                }
            }
            if (ok) *reinterpret_cast<V*>(out + (int64_t)r * ldo + c0) = s;
        }
    }
}

}  // namespace

extern "C" size_t sage_csr_sum_workspace_bytes(int64_t num_rows, int64_t max_edges, int32_t dim) {
    SumLayout L;
    return sum_layout(num_rows, max_edges, dim, &L) ? L.total : 0;
}

extern "C" int sage_csr_sum(const int64_t* rowptr, const int32_t* col, int64_t num_rows, int64_t max_edges, const float* table,
                            int64_t table_rows, int64_t ld, int32_t dim, float* out, int64_t ldo, void* workspace, size_t workspace_bytes,
                            sage_stream_t stream) {
    // shapes first, then pointers: a bad shape is reported as such whatever the pointers are
    SAGE_REQUIRE(num_rows >= 0 && num_rows < (1ll << 31), "csr_sum: num_rows = %lld", (long long)num_rows);
    SAGE_REQUIRE(max_edges >= 0, "csr_sum: max_edges = %lld", (long long)max_edges);
    SAGE_REQUIRE(dim >= 1 && ld >= dim && ldo >= dim, "csr_sum: dim = %d, ld = %lld, ldo = %lld", dim, (long long)ld, (long long)ldo);
    SAGE_REQUIRE(table_rows >= 1 && table_rows < (1ll << 31), "csr_sum: table_rows = %lld", (long long)table_rows);
    SumLayout L;
    SAGE_REQUIRE(sum_layout(num_rows, max_edges, dim, &L), "csr_sum: num_rows = %lld, max_edges = %lld, dim = %d out of range",
                 (long long)num_rows, (long long)max_edges, dim);
    SAGE_REQUIRE(rowptr && col && table && out, "csr_sum: NULL array");
    if (workspace_bytes < L.total || !workspace) {
        sage_set_error("csr_sum: workspace of %zu bytes, %zu needed", workspace_bytes, L.total);
        return SAGE_ENOSPACE;
    }
    SAGE_REQUIRE(sage_aligned(workspace, 256), "csr_sum: workspace not 256-byte aligned");
    if (num_rows == 0) return SAGE_OK;
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace;
    int64_t* off = (int64_t*)(ws + L.off);
    int64_t* carry = (int64_t*)(ws + L.carry);
    int32_t* item_row = (int32_t*)(ws + L.item_row);
    float* partials = (float*)(ws + L.partials);
    const int n = (int)num_rows, nb = (int)L.nblocks;

    hipLaunchKernelGGL(csr_count_kernel, dim3(nb), dim3(kCountThreads), 0, st, rowptr, num_rows, (const int32_t*)nullptr, n, off, carry);
    SAGE_CHECK_LAUNCH("csr_count_kernel");
    hipLaunchKernelGGL(csr_carry_kernel, dim3(1), dim3(kCarryThreads), 0, st, carry, nb);
    SAGE_CHECK_LAUNCH("csr_carry_kernel");
    hipLaunchKernelGGL(csr_expand_kernel, dim3(sage_cdiv(n, 256)), dim3(256), 0, st, rowptr, num_rows, (const int32_t*)nullptr, n, off, carry,
                       L.cap, item_row);
    SAGE_CHECK_LAUNCH("csr_expand_kernel");

    const bool vec4 = (dim % 4 == 0) && (ld % 4 == 0) && (ldo % 4 == 0) && sage_aligned(table, 16) && sage_aligned(out, 16);
    if (L.cap > 0) {
        const int blocks = (int)std::min<int64_t>((L.cap + 3) / 4, kNumCU * 8);
        if (vec4)
            hipLaunchKernelGGL(sum_chunk_kernel<4>, dim3(blocks), dim3(256), 0, st, rowptr, col, num_rows, table, (int)table_rows, ld, dim, off,
                               carry, nb, L.cap, item_row, partials);
        else
            hipLaunchKernelGGL(sum_chunk_kernel<1>, dim3(blocks), dim3(256), 0, st, rowptr, col, num_rows, table, (int)table_rows, ld, dim, off,
                               carry, nb, L.cap, item_row, partials);
        SAGE_CHECK_LAUNCH("sum_chunk_kernel");
    }
    const int blocks = std::min(sage_cdiv(n, 4), kNumCU * 8);
    if (vec4)
        hipLaunchKernelGGL(sum_row_kernel<4>, dim3(blocks), dim3(256), 0, st, rowptr, col, num_rows, table, (int)table_rows, ld, dim, off, L.cap,
                           partials, out, ldo);
    else
        hipLaunchKernelGGL(sum_row_kernel<1>, dim3(blocks), dim3(256), 0, st, rowptr, col, num_rows, table, (int)table_rows, ld, dim, off, L.cap,
                           partials, out, ldo);
    SAGE_CHECK_LAUNCH("sum_row_kernel");
    return SAGE_OK;
}
