// csr_mean: per-row mean over a node's WHOLE CSR neighbourhood (aggregators.py:47-48 num_sample=None, then 52-74).
//
// The fixed-fanout gathers read a padded [n, k] list and give each row to one wave.  A full neighbourhood is skewed
// (configs[2]'s graph: max degree 62,333 against a median of 1), and one wave per row then runs as long as its hub.
// Split rule (cdna_hip_programming.md Appendix B, "Scatter / gather / embedding"): a row is cut into chunks of
// SAGE_CSR_MEAN_CHUNK edges; rows of one chunk are finished in place, longer rows have each chunk summed by a wave of
// its own into a workspace partial, and a later pass adds a row's partials in chunk order.
//
// Launches, all on the caller's stream, no host round trip:
//   1. count   per row: chunks of the row if it is long (else 0); block-local exclusive offsets + one sum per block
//   2. carry   one block: exclusive scan of the block sums (the total lands at carry[nblocks])
//   3. expand  global chunk offset of every long row; its chunks' item entries (item -> row)
//   4. chunk   one wave per item: the chunk's partial sum (and whether the chunk holds the row's own node)
//   5. rows    one wave per row: short rows summed in place; long rows = their partials in chunk order
// The item list is sized on the host from max_edges.  A caller whose bound is too small costs speed only: a long row
// whose chunks do not fit is summed chunk by chunk by its row wave, with the same operations in the same order.
//
// Arithmetic of a row (its bits depend on nothing else): p_c = 0 + t_0 + t_1 + ... over chunk c's edges in CSR order;
// S = 0 + p_0 + p_1 + ...; S += self row (set union, aggregators.py:50-51); out = S * (1 / count).
//
// IDX instantiations (sage_csr_mean_indexed): the table is virtual, T[v] = embed[index[v]] (aggregators.py:68-71), and only the
// ADDRESS of a row changes: the lane that loads col[base + lane] also loads index[] of the clamped id, the self row is read
// through index[v].  "Row v holds v" is still decided on node ids.  Same chunks, launches, fall-back and order of additions.
#include "sage_csr_common.h"

namespace {

struct CsrLayout {
    size_t off, carry, item_row, has_self, partials, total;
    int64_t cap;       // item entries (= partial rows) the workspace holds
    int64_t nblocks;   // count-kernel blocks
};

bool csr_layout(int32_t n, int64_t max_edges, int32_t dim, CsrLayout* L) {
    if (n < 0 || max_edges < 0 || dim < 1) return false;
    L->cap = csr_item_cap(n, max_edges);
    if (L->cap >= (1ll << 31)) return false;
    L->nblocks = ((int64_t)n + kCountTile - 1) / kCountTile;
    size_t off = 0;
    auto take = [&](size_t bytes) { size_t o = off; off = align256(off + std::max<size_t>(bytes, 1)); return o; };
    L->off = take((size_t)n * 8);
    L->carry = take((size_t)(L->nblocks + 1) * 8);
    L->item_row = take((size_t)L->cap * 4);
    L->has_self = take((size_t)L->cap * 4);
    L->partials = take((size_t)L->cap * (size_t)dim * 4);
    L->total = off;
    return true;
}

// acc += table rows of col[b..e) in edge order (the sage_gather.hip inner loop: ids broadcast by readlane, 8 rows in flight).
// b, e wave-uniform.  found |= some edge of the range is node v.
// IDX: the id is a node id, clamped into [0, last_node]; the row read is index[id], clamped into [0, last_row].
template <int VEC, bool IDX>
__device__ inline void sum_edges(const int32_t* __restrict__ col, int64_t b, int64_t e, const float* __restrict__ table, int64_t ld,
                                 int last_row, int c0, bool ok, int32_t v, typename VecT<VEC>::type& acc, bool& found,
                                 const int32_t* __restrict__ index, int last_node) {
    using V = typename VecT<VEC>::type;
    const int lane = sage_lane();
    for (int64_t base = b; base < e; base += kWave) {
        const int m = (int)min((int64_t)kWave, e - base);
        const int raw = (lane < m) ? col[base + lane] : -1;
        if (__any(lane < m && raw == v)) found = true;
        int myid;
        if constexpr (IDX) {
            const int node = min(max(raw, 0), last_node);                            // never read outside index[]
            myid = min(max(lane < m ? index[node] : 0, 0), last_row);                // ... nor outside embed[]
        } else {
            myid = min(max(raw, 0), last_row);           // never read outside the table
        }
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

// 4. one wave per item (row, chunk): partials[item] := the chunk's sum, has_self[item] := the chunk holds node v
template <int VEC, bool IDX>
__global__ __launch_bounds__(256) void csr_chunk_kernel(const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col, int64_t num_nodes,
                                                        const int32_t* __restrict__ nodes, int n, const float* __restrict__ table,
                                                        int table_rows, int64_t ld, int dim, const int64_t* __restrict__ off,
                                                        const int64_t* __restrict__ carry, int nb, int64_t cap,
                                                        const int32_t* __restrict__ item_row, int32_t* __restrict__ has_self,
                                                        float* __restrict__ partials, const int32_t* __restrict__ index) {
    using V = typename VecT<VEC>::type;
    const int lane = sage_lane();
    const int64_t wave = (int64_t)((blockIdx.x * blockDim.x + threadIdx.x) >> 6);
    const int64_t nwaves = (int64_t)((gridDim.x * blockDim.x) >> 6);
    const int64_t items = min(carry[nb], cap);
    const int64_t total = rowptr[num_nodes];
    for (int64_t i = wave; i < items; i += nwaves) {
        // With a max_edges below the truth the entries of a row that did not fit were never written: take an entry only if
        // it names a row whose chunk range fits and holds i (the ranges are disjoint, so a stale value cannot pass)
        const int r = __builtin_amdgcn_readfirstlane(item_row[i]);
        if (r < 0 || r >= n) continue;
        int32_t v;
        int64_t b, e;
        row_span(rowptr, num_nodes, nodes, r, total, v, b, e);
        v = __builtin_amdgcn_readfirstlane(v);
        b = uniform64(b);
        e = uniform64(e);
        const int64_t k = long_chunks(e - b), o = uniform64(off[r]);
        if (k == 0 || o + k > cap || i < o || i >= o + k) continue;
        const int64_t cb = b + (i - o) * kChunk;
        const int64_t ce = min(cb + kChunk, e);
        bool found = false;
        for (int cbk = 0; cbk < dim; cbk += kWave * VEC) {
            const int c0 = cbk + lane * VEC;
            const bool ok = c0 < dim;
            V acc;
            vfill(acc, 0.f);
            sum_edges<VEC, IDX>(col, cb, ce, table, ld, table_rows - 1, c0, ok, v, acc, found, index, (int)num_nodes - 1);
            if (ok) *reinterpret_cast<V*>(partials + i * dim + c0) = acc;
        }
        if (lane == 0) has_self[i] = found ? 1 : 0;
    }
}

// 5. one wave per row
template <int VEC, bool IDX>
__global__ __launch_bounds__(256) void csr_row_kernel(const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col, int64_t num_nodes,
                                                      const int32_t* __restrict__ nodes, int n, const float* __restrict__ table,
                                                      int table_rows, int64_t ld, int dim, int self_loop,
                                                      const int32_t* __restrict__ any_nonempty, const int64_t* __restrict__ off,
                                                      int64_t cap, const int32_t* __restrict__ has_self,
                                                      const float* __restrict__ partials, float* __restrict__ out, int64_t ldo,
                                                      const int32_t* __restrict__ index) {
    using V = typename VecT<VEC>::type;
    const int lane = sage_lane();
    const int wave = (int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6);
    const int nwaves = (int)((gridDim.x * blockDim.x) >> 6);
    const bool nan_rule = any_nonempty ? (*any_nonempty != 0) : false;
    const int last_row = table_rows - 1;
    const int last_node = (int)num_nodes - 1;
    const int64_t total = rowptr[num_nodes];
    for (int r = wave; r < n; r += nwaves) {
        int32_t v;
        int64_t b, e;
        row_span(rowptr, num_nodes, nodes, r, total, v, b, e);
        v = __builtin_amdgcn_readfirstlane(v);
        b = uniform64(b);
        e = uniform64(e);
        const int64_t deg = e - b;
        const int64_t k = long_chunks(deg);
        const int64_t o = k > 0 ? uniform64(off[r]) : 0;
        const bool split = k > 0 && o + k <= cap;        // the chunk pass summed this row's chunks
        bool found = false;
        if (split) {
            bool f = false;
            for (int64_t c = lane; c < k; c += kWave) f |= has_self[o + c] != 0;
            found = __any(f);
        }
        for (int cb = 0; cb < dim; cb += kWave * VEC) {
            const int c0 = cb + lane * VEC;
            const bool ok = c0 < dim;
            V s;
            vfill(s, 0.f);
            if (split) {
                if (ok)
                    for (int64_t c = 0; c < k; ++c) vadd(s, *reinterpret_cast<const V*>(partials + (o + c) * dim + c0));
            } else if (k == 0) {
                sum_edges<VEC, IDX>(col, b, e, table, ld, last_row, c0, ok, v, s, found, index, last_node);
            } else {                                      // long row without workspace room: the chunk pass's sums, here
                for (int64_t c = 0; c < k; ++c) {
                    V p;
                    vfill(p, 0.f);
                    sum_edges<VEC, IDX>(col, b + c * kChunk, min(b + (c + 1) * kChunk, e), table, ld, last_row, c0, ok, v, p, found, index,
                                        last_node);
                    vadd(s, p);
                }
            }
            const bool extra = self_loop && v >= 0 && !found;   // aggregators.py:50-51: set union
            if (extra && ok) {
                int self;                                       // v is in [0, num_nodes) here
                if constexpr (IDX) self = min(max(__builtin_amdgcn_readfirstlane(index[v]), 0), last_row);
                else self = min(v, last_row);
                vadd(s, *reinterpret_cast<const V*>(table + (int64_t)self * ld + c0));
            }
            const int64_t ceff = deg + (extra ? 1 : 0);
            if (ok) {
                V res;
                if (ceff > 0) res = vscale(s, 1.0f / (float)ceff);
                else vfill(res, nan_rule ? __builtin_nanf("") : 0.f);
                *reinterpret_cast<V*>(out + (int64_t)r * ldo + c0) = res;
            }
        }
    }
}

}  // namespace

extern "C" size_t sage_csr_mean_workspace_bytes(int32_t n, int64_t max_edges, int32_t dim) {
    CsrLayout L;
    return csr_layout(n, max_edges, dim, &L) ? L.total : 0;
}

// The five launches, for the plain table (index == nullptr) and for the virtual one.  Arguments are validated by the entries.
static int csr_mean_launch(const int64_t* rowptr, const int32_t* col, int64_t num_nodes, const int32_t* nodes, int32_t n,
                           const int32_t* index, const float* table, int64_t table_rows, int64_t ld, int32_t dim, int32_t self_loop,
                           const int32_t* any_nonempty, float* out, int64_t ldo, void* workspace, const CsrLayout& L,
                           sage_stream_t stream) {
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace;
    int64_t* off = (int64_t*)(ws + L.off);
    int64_t* carry = (int64_t*)(ws + L.carry);
    int32_t* item_row = (int32_t*)(ws + L.item_row);
    int32_t* has_self = (int32_t*)(ws + L.has_self);
    float* partials = (float*)(ws + L.partials);
    const int nb = (int)L.nblocks;

    hipLaunchKernelGGL(csr_count_kernel, dim3(nb), dim3(kCountThreads), 0, st, rowptr, num_nodes, nodes, n, off, carry);
    SAGE_CHECK_LAUNCH("csr_count_kernel");
    hipLaunchKernelGGL(csr_carry_kernel, dim3(1), dim3(kCarryThreads), 0, st, carry, nb);
    SAGE_CHECK_LAUNCH("csr_carry_kernel");
    hipLaunchKernelGGL(csr_expand_kernel, dim3(sage_cdiv(n, 256)), dim3(256), 0, st, rowptr, num_nodes, nodes, n, off, carry, L.cap, item_row);
    SAGE_CHECK_LAUNCH("csr_expand_kernel");

    const bool vec4 = (dim % 4 == 0) && (ld % 4 == 0) && (ldo % 4 == 0) && sage_aligned(table, 16) && sage_aligned(out, 16);
    if (L.cap > 0) {
        const int blocks = (int)std::min<int64_t>((L.cap + 3) / 4, kNumCU * 8);
#define SAGE_CSR_CHUNK(VEC, IDX)                                                                                                       \
    hipLaunchKernelGGL((csr_chunk_kernel<VEC, IDX>), dim3(blocks), dim3(256), 0, st, rowptr, col, num_nodes, nodes, n, table, (int)table_rows, \
                       ld, dim, off, carry, nb, L.cap, item_row, has_self, partials, index)
        if (index) { if (vec4) SAGE_CSR_CHUNK(4, true); else SAGE_CSR_CHUNK(1, true); }
        else { if (vec4) SAGE_CSR_CHUNK(4, false); else SAGE_CSR_CHUNK(1, false); }
#undef SAGE_CSR_CHUNK
        SAGE_CHECK_LAUNCH("csr_chunk_kernel");
    }
    const int blocks = std::min(sage_cdiv(n, 4), kNumCU * 8);
#define SAGE_CSR_ROW(VEC, IDX)                                                                                                            \
    hipLaunchKernelGGL((csr_row_kernel<VEC, IDX>), dim3(blocks), dim3(256), 0, st, rowptr, col, num_nodes, nodes, n, table, (int)table_rows, ld, \
                       dim, self_loop, any_nonempty, off, L.cap, has_self, partials, out, ldo, index)
    if (index) { if (vec4) SAGE_CSR_ROW(4, true); else SAGE_CSR_ROW(1, true); }
    else { if (vec4) SAGE_CSR_ROW(4, false); else SAGE_CSR_ROW(1, false); }
#undef SAGE_CSR_ROW
    SAGE_CHECK_LAUNCH("csr_row_kernel");
    return SAGE_OK;
}

extern "C" int sage_csr_mean(const int64_t* rowptr, const int32_t* col, int64_t num_nodes, const int32_t* nodes, int32_t n,
                             int64_t max_edges, const float* table, int64_t table_rows, int64_t ld, int32_t dim, int32_t self_loop,
                             const int32_t* any_nonempty, float* out, int64_t ldo, void* workspace, size_t workspace_bytes,
                             sage_stream_t stream) {
    // shapes first, then pointers: a bad shape is reported as such whatever the pointers are
    SAGE_REQUIRE(num_nodes >= 0 && num_nodes < (1ll << 31), "csr_mean: num_nodes = %lld", (long long)num_nodes);
    SAGE_REQUIRE(n >= 0 && (nodes || n <= num_nodes), "csr_mean: n = %d rows for %lld nodes without a node list", n, (long long)num_nodes);
    SAGE_REQUIRE(max_edges >= 0, "csr_mean: max_edges = %lld", (long long)max_edges);
    SAGE_REQUIRE(dim >= 1 && ld >= dim && ldo >= dim, "csr_mean: dim = %d, ld = %lld, ldo = %lld", dim, (long long)ld, (long long)ldo);
    SAGE_REQUIRE(table_rows >= 1 && table_rows < (1ll << 31), "csr_mean: table_rows = %lld", (long long)table_rows);
    SAGE_REQUIRE(self_loop == 0 || self_loop == 1, "csr_mean: self_loop = %d", self_loop);
    SAGE_REQUIRE(rowptr && col && table && out, "csr_mean: NULL array");
    CsrLayout L;
    SAGE_REQUIRE(csr_layout(n, max_edges, dim, &L), "csr_mean: n = %d, max_edges = %lld, dim = %d out of range", n, (long long)max_edges, dim);
    if (workspace_bytes < L.total || !workspace) {
        sage_set_error("csr_mean: workspace of %zu bytes, %zu needed", workspace_bytes, L.total);
        return SAGE_ENOSPACE;
    }
    SAGE_REQUIRE(sage_aligned(workspace, 256), "csr_mean: workspace not 256-byte aligned");
    if (n == 0) return SAGE_OK;
    return csr_mean_launch(rowptr, col, num_nodes, nodes, n, nullptr, table, table_rows, ld, dim, self_loop, any_nonempty, out, ldo, workspace, L,
                           stream);
}

extern "C" int sage_csr_mean_indexed(const int64_t* rowptr, const int32_t* col, int64_t num_nodes, const int32_t* nodes, int32_t n,
                                     int64_t max_edges, const int32_t* index, const float* embed, int64_t embed_rows, int64_t ld, int32_t dim,
                                     int32_t self_loop, const int32_t* any_nonempty, float* out, int64_t ldo, void* workspace,
                                     size_t workspace_bytes, sage_stream_t stream) {
    // shapes first, then pointers, then the workspace: sage_csr_mean's order
    SAGE_REQUIRE(num_nodes >= 0 && num_nodes < (1ll << 31), "csr_mean_indexed: num_nodes = %lld", (long long)num_nodes);
    SAGE_REQUIRE(n >= 0 && (nodes || n <= num_nodes), "csr_mean_indexed: n = %d rows for %lld nodes without a node list", n,
                 (long long)num_nodes);
    SAGE_REQUIRE(max_edges >= 0, "csr_mean_indexed: max_edges = %lld", (long long)max_edges);
    SAGE_REQUIRE(dim >= 1 && ld >= dim && ldo >= dim, "csr_mean_indexed: dim = %d, ld = %lld, ldo = %lld", dim, (long long)ld, (long long)ldo);
    SAGE_REQUIRE(embed_rows >= 1 && embed_rows < (1ll << 31), "csr_mean_indexed: embed_rows = %lld", (long long)embed_rows);
    SAGE_REQUIRE(self_loop == 0 || self_loop == 1, "csr_mean_indexed: self_loop = %d", self_loop);
    SAGE_REQUIRE(rowptr && col && index && embed && out, "csr_mean_indexed: NULL array");
    CsrLayout L;
    SAGE_REQUIRE(csr_layout(n, max_edges, dim, &L), "csr_mean_indexed: n = %d, max_edges = %lld, dim = %d out of range", n,
                 (long long)max_edges, dim);
    if (workspace_bytes < L.total || !workspace) {
        sage_set_error("csr_mean_indexed: workspace of %zu bytes, %zu needed", workspace_bytes, L.total);
        return SAGE_ENOSPACE;
    }
    SAGE_REQUIRE(sage_aligned(workspace, 256), "csr_mean_indexed: workspace not 256-byte aligned");
    if (n == 0) return SAGE_OK;
    return csr_mean_launch(rowptr, col, num_nodes, nodes, n, index, embed, embed_rows, ld, dim, self_loop, any_nonempty, out, ldo, workspace, L,
                           stream);
}
