// csr_sum: per-row SUM of table rows over a rectangular CSR (num_rows groups over table_rows source rows) -- the reduction
// behind the gradient of a shared embedding row (aggregators.py:68-71: every node of one index reads one row of `embed`):
//     grad_embed[k] = sum over the nodes v with index[v] = k of grad_X[v]
// The grouping (rowptr, col) is built once per graph (ops.group_rows).  Its row lengths are the histogram of the index -- for
// node_degree the degree histogram of a power-law graph: a few rows hold most of the nodes, most rows are empty -- so this is
// sage_csr_mean's split (sage_csr_mean.hip) without its division, self term and NaN rule:
//   1-3. count, carry, expand (sage_csr_common.h: csr_chunk_plan)
//   4. chunk   one wave per item: partials[item] := the sum of the chunk's SAGE_CSR_MEAN_CHUNK entries
//   5. rows    one wave per row: short rows summed in place; long rows = their partials in chunk order; store
// A long row whose chunks do not fit the workspace is summed chunk by chunk by its row wave, with the same operations in the
// same order.  No float atomics; every row of out is stored, an empty row as zeros.
//
// Arithmetic of a row (its bits depend on nothing else): p_c = 0 + t_0 + t_1 + ... over chunk c's entries in stored order;
// out[r] = 0 + p_0 + p_1 + ... for a row of more than one chunk, out[r] = p_0 for any other.  Both live in sage_csr_common.h: the
// terms are sum_edges' (sage_csr_mean.hip's walker with the self test compiled out), the row's total is chunked_row_sum's.
#include "sage_csr_common.h"

namespace {

struct SumLayout {
    ChunkWs c;
    size_t total;
};

bool sum_layout(int64_t num_rows, int64_t max_edges, int32_t dim, SumLayout* L) {
    if (num_rows < 0 || num_rows >= (1ll << 31) || max_edges < 0 || dim < 1) return false;
    WsCursor cur;
    if (!chunk_ws(num_rows, max_edges, dim, cur, &L->c)) return false;
    L->total = cur.off;
    return true;
}

// acc += table rows of col[b..e) in stored order, ids clamped into the table: sum_edges without an index and without the self test
template <int VEC>
__device__ inline void sum_terms(const int32_t* __restrict__ col, int64_t b, int64_t e, const float* __restrict__ table, int64_t ld,
                                 int last_row, int c0, bool ok, typename VecT<VEC>::type& acc) {
    bool unused = false;
    sum_edges<VEC, false, false>(col, b, e, table, ld, last_row, c0, ok, -1, acc, unused, nullptr, 0);
}

// 4. one wave per item (row, chunk): partials[item] := the chunk's sum
template <int VEC>
__global__ __launch_bounds__(256) void sum_chunk_kernel(const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col, int64_t num_rows,
                                                        const float* __restrict__ table, int table_rows, int64_t ld, int dim,
                                                        const int64_t* __restrict__ off, const int64_t* __restrict__ carry, int nb,
                                                        int64_t cap, const int32_t* __restrict__ item_row, float* __restrict__ partials) {
    using V = typename VecT<VEC>::type;
    const int lane = sage_lane();
    const int64_t wave = (int64_t)((blockIdx.x * blockDim.x + threadIdx.x) >> 6);
    const int64_t nwaves = (int64_t)((gridDim.x * blockDim.x) >> 6);
    const int64_t items = min(carry[nb], cap);
    const int64_t total = rowptr[num_rows];
    for (int64_t i = wave; i < items; i += nwaves) {
        int32_t v;
        int64_t cb, ce;
        if (!chunk_item<true>(i, item_row, rowptr, num_rows, nullptr, (int)num_rows, total, off, cap, v, cb, ce)) continue;
        for (int cbk = 0; cbk < dim; cbk += kWave * VEC) {
            const int c0 = cbk + lane * VEC;
            const bool ok = c0 < dim;
            V acc;
            vfill(acc, 0.f);
            sum_terms<VEC>(col, cb, ce, table, ld, table_rows - 1, c0, ok, acc);
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
        row_span<true>(rowptr, num_rows, nullptr, r, total, v, b, e);
        const int64_t k = long_chunks(e - b);
        const int64_t o = first_item<true>(off, r, k);
        for (int cb = 0; cb < dim; cb += kWave * VEC) {
            const int c0 = cb + lane * VEC;
            const bool ok = c0 < dim;
            const V s = chunked_row_sum<V>(k, o, cap, partials, dim, c0, ok, b, e, [&](int64_t tb, int64_t te, V& acc) {
                sum_terms<VEC>(col, tb, te, table, ld, last_row, c0, ok, acc);
            });
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
    if (const int rc = csr_workspace_check("csr_sum", workspace, workspace_bytes, L.total)) return rc;
    if (num_rows == 0) return SAGE_OK;
    hipStream_t st = (hipStream_t)stream;
    const int n = (int)num_rows;
    ChunkPlan P;
    if (const int rc = csr_chunk_plan(rowptr, num_rows, nullptr, n, workspace, L.c, st, &P)) return rc;

    const bool vec4 = (dim % 4 == 0) && (ld % 4 == 0) && (ldo % 4 == 0) && sage_aligned(table, 16) && sage_aligned(out, 16);
    if (P.cap > 0) {
        const int blocks = (int)std::min<int64_t>((P.cap + 3) / 4, kNumCU * 8);
        if (vec4)
            hipLaunchKernelGGL(sum_chunk_kernel<4>, dim3(blocks), dim3(256), 0, st, rowptr, col, num_rows, table, (int)table_rows, ld, dim, P.off,
                               P.carry, P.nb, P.cap, P.item_row, P.partials);
        else
            hipLaunchKernelGGL(sum_chunk_kernel<1>, dim3(blocks), dim3(256), 0, st, rowptr, col, num_rows, table, (int)table_rows, ld, dim, P.off,
                               P.carry, P.nb, P.cap, P.item_row, P.partials);
        SAGE_CHECK_LAUNCH("sum_chunk_kernel");
    }
    const int blocks = std::min(sage_cdiv(n, 4), kNumCU * 8);
    if (vec4)
        hipLaunchKernelGGL(sum_row_kernel<4>, dim3(blocks), dim3(256), 0, st, rowptr, col, num_rows, table, (int)table_rows, ld, dim, P.off, P.cap,
                           P.partials, out, ldo);
    else
        hipLaunchKernelGGL(sum_row_kernel<1>, dim3(blocks), dim3(256), 0, st, rowptr, col, num_rows, table, (int)table_rows, ld, dim, P.off, P.cap,
                           P.partials, out, ldo);
    SAGE_CHECK_LAUNCH("sum_row_kernel");
    return SAGE_OK;
}
