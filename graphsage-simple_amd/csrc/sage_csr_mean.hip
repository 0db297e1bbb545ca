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
// Launches 1-3, the item check of launch 4 and the three ways launch 5 totals a row are sage_csr_common.h's (csr_chunk_plan,
// chunk_item, chunked_row_sum), shared with sage_csr_sum.hip, sage_csr_mean_backward.hip and sage_embed_grad.hip; this file owns the
// has_self flags and what follows a row's total.
//
// Arithmetic of a row (its bits depend on nothing else): p_c = 0 + t_0 + t_1 + ... over chunk c's edges in CSR order (sum_edges);
// S = 0 + p_0 + p_1 + ... (chunked_row_sum); S += self row (set union, aggregators.py:50-51); out = S * (1 / count).
//
// IDX instantiations (sage_csr_mean_indexed): the table is virtual, T[v] = embed[index[v]] (aggregators.py:68-71), and only the
// ADDRESS of a row changes: the lane that loads col[base + lane] also loads index[] of the clamped id, the self row is read
// through index[v].  "Row v holds v" is still decided on node ids.  Same chunks, launches, fall-back and order of additions.
//
// TT = uint16_t instantiations (sage_csr_mean_bf16): the frozen table is STORED as bf16.  Only the LOAD of a table element changes
// (load_cols: 8 bytes for a lane's four columns, widened exactly by `<< 16` / `& 0xffff0000`); accumulators, partials and out stay
// fp32 with the layout above, so the result is the fp32 kernel's on the widened table bit for bit.  No IDX form.
#include "sage_csr_common.h"

#ifndef SAGE_CSR_BF16_COLS
#define SAGE_CSR_BF16_COLS 4
#endif

namespace {

struct CsrLayout {
    ChunkWs c;
    size_t has_self, total;
};

bool csr_layout(int32_t n, int64_t max_edges, int32_t dim, CsrLayout* L) {
    if (n < 0 || max_edges < 0 || dim < 1) return false;
    WsCursor cur;
    if (!chunk_ws(n, max_edges, dim, cur, &L->c)) return false;
    L->has_self = cur.take((size_t)L->c.cap * 4);
    L->total = cur.off;
    return true;
}

// 4. one wave per item (row, chunk): partials[item] := the chunk's sum, has_self[item] := the chunk holds node v
template <int VEC, bool IDX, typename TT>
__global__ __launch_bounds__(256) void csr_chunk_kernel(const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col, int64_t num_nodes,
                                                        const int32_t* __restrict__ nodes, int n, const TT* __restrict__ table,
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
        int32_t v;
        int64_t cb, ce;
        if (!chunk_item<true>(i, item_row, rowptr, num_nodes, nodes, n, total, off, cap, v, cb, ce)) continue;
        bool found = false;
        for (int cbk = 0; cbk < dim; cbk += kWave * VEC) {
            const int c0 = cbk + lane * VEC;
            const bool ok = c0 < dim;
            V acc;
            vfill(acc, 0.f);
            sum_edges<VEC, IDX, true>(col, cb, ce, table, ld, table_rows - 1, c0, ok, v, acc, found, index, (int)num_nodes - 1);
            if (ok) *reinterpret_cast<V*>(partials + i * dim + c0) = acc;
        }
        if (lane == 0) has_self[i] = found ? 1 : 0;
    }
}

// 5. one wave per row
template <int VEC, bool IDX, typename TT>
__global__ __launch_bounds__(256) void csr_row_kernel(const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col, int64_t num_nodes,
                                                      const int32_t* __restrict__ nodes, int n, const TT* __restrict__ table,
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
        row_span<true>(rowptr, num_nodes, nodes, r, total, v, b, e);
        const int64_t deg = e - b;
        const int64_t k = long_chunks(deg);
        const int64_t o = first_item<true>(off, r, k);
        bool found = false;
        if (chunks_fit(k, o, cap)) {                     // the chunk pass looked for node v in this row's chunks
            bool f = false;
            for (int64_t c = lane; c < k; c += kWave) f |= has_self[o + c] != 0;
            found = __any(f);
        }
        for (int cb = 0; cb < dim; cb += kWave * VEC) {
            const int c0 = cb + lane * VEC;
            const bool ok = c0 < dim;
            V s = chunked_row_sum<V>(k, o, cap, partials, dim, c0, ok, b, e, [&](int64_t tb, int64_t te, V& acc) {
                sum_edges<VEC, IDX, true>(col, tb, te, table, ld, last_row, c0, ok, v, acc, found, index, last_node);
            });
            const bool extra = self_loop && v >= 0 && !found;   // aggregators.py:50-51: set union
            if (extra && ok) {
                int self;                                       // v is in [0, num_nodes) here
                if constexpr (IDX) self = min(max(__builtin_amdgcn_readfirstlane(index[v]), 0), last_row);
                else self = min(v, last_row);
                vadd(s, load_cols<V>(table + (int64_t)self * ld + c0));
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

// All three entries: the refusals (shapes first, then pointers, then the workspace: a bad shape is reported as such whatever the pointers
// are) under the entry's `name` and its word for the table's rows, then the five launches, for the plain table (index == nullptr,
// indexed false) and for the virtual one.  TT = uint16_t: the plain table stored as bf16 (no indexed form: the embedding it would
// read is trained, and stays fp32); ld counts elements, and the vector path's one load per lane is 8 bytes.
template <typename TT>
static int csr_mean_run(const char* name, const char* rows_name, bool indexed, const int64_t* rowptr, const int32_t* col, int64_t num_nodes,
                        const int32_t* nodes, int32_t n, int64_t max_edges, const int32_t* index, const TT* table, int64_t table_rows,
                        int64_t ld, int32_t dim, int32_t self_loop, const int32_t* any_nonempty, float* out, int64_t ldo, void* workspace,
                        size_t workspace_bytes, sage_stream_t stream) {
    SAGE_REQUIRE(num_nodes >= 0 && num_nodes < (1ll << 31), "%s: num_nodes = %lld", name, (long long)num_nodes);
    SAGE_REQUIRE(n >= 0 && (nodes || n <= num_nodes), "%s: n = %d rows for %lld nodes without a node list", name, n, (long long)num_nodes);
    SAGE_REQUIRE(max_edges >= 0, "%s: max_edges = %lld", name, (long long)max_edges);
    SAGE_REQUIRE(dim >= 1 && ld >= dim && ldo >= dim, "%s: dim = %d, ld = %lld, ldo = %lld", name, dim, (long long)ld, (long long)ldo);
    SAGE_REQUIRE(table_rows >= 1 && table_rows < (1ll << 31), "%s: %s = %lld", name, rows_name, (long long)table_rows);
    SAGE_REQUIRE(self_loop == 0 || self_loop == 1, "%s: self_loop = %d", name, self_loop);
    SAGE_REQUIRE(rowptr && col && (index || !indexed) && table && out, "%s: NULL array", name);
    CsrLayout L;
    SAGE_REQUIRE(csr_layout(n, max_edges, dim, &L), "%s: n = %d, max_edges = %lld, dim = %d out of range", name, n, (long long)max_edges, dim);
    if (const int rc = csr_workspace_check(name, workspace, workspace_bytes, L.total)) return rc;
    if (n == 0) return SAGE_OK;

    hipStream_t st = (hipStream_t)stream;
    ChunkPlan P;
    if (const int rc = csr_chunk_plan(rowptr, num_nodes, nodes, n, workspace, L.c, st, &P)) return rc;
    int32_t* has_self = (int32_t*)((char*)workspace + L.has_self);
    constexpr bool kIsFloat = std::is_same_v<TT, float>;
    const bool vec4 = (dim % 4 == 0) && (ld % 4 == 0) && (ldo % 4 == 0) && sage_aligned(table, 4 * sizeof(TT)) && sage_aligned(out, 16);
    // the bf16 table's 16-byte form, eight columns per lane: built with -DSAGE_CSR_BF16_COLS=8 only (experiments/mb_csr_mean_bf16.py);
    // it lost to the 8-byte form, so the library holds no such kernel
    constexpr bool kCols8 = !kIsFloat && SAGE_CSR_BF16_COLS == 8;
    const bool vec8 = kCols8 && vec4 && (dim % 8 == 0) && (ld % 8 == 0) && sage_aligned(table, 16);
    if (P.cap > 0) {
        const int blocks = (int)std::min<int64_t>((P.cap + 3) / 4, kNumCU * 8);
#define SAGE_CSR_CHUNK(VEC, IDX)                                                                                                       \
    hipLaunchKernelGGL((csr_chunk_kernel<VEC, IDX, TT>), dim3(blocks), dim3(256), 0, st, rowptr, col, num_nodes, nodes, n, table, (int)table_rows, \
                       ld, dim, P.off, P.carry, P.nb, P.cap, P.item_row, has_self, P.partials, index)
        bool launched = false;
        if constexpr (kIsFloat)
            if (index) { if (vec4) SAGE_CSR_CHUNK(4, true); else SAGE_CSR_CHUNK(1, true); launched = true; }
        if constexpr (kCols8)
            if (vec8) { SAGE_CSR_CHUNK(8, false); launched = true; }
        if (!launched) { if (vec4) SAGE_CSR_CHUNK(4, false); else SAGE_CSR_CHUNK(1, false); }
#undef SAGE_CSR_CHUNK
        SAGE_CHECK_LAUNCH("csr_chunk_kernel");
    }
    const int blocks = std::min(sage_cdiv(n, 4), kNumCU * 8);
#define SAGE_CSR_ROW(VEC, IDX)                                                                                                            \
    hipLaunchKernelGGL((csr_row_kernel<VEC, IDX, TT>), dim3(blocks), dim3(256), 0, st, rowptr, col, num_nodes, nodes, n, table, (int)table_rows, ld, \
                       dim, self_loop, any_nonempty, P.off, P.cap, has_self, P.partials, out, ldo, index)
    bool launched = false;
    if constexpr (kIsFloat)
        if (index) { if (vec4) SAGE_CSR_ROW(4, true); else SAGE_CSR_ROW(1, true); launched = true; }
    if constexpr (kCols8)
        if (vec8) { SAGE_CSR_ROW(8, false); launched = true; }
    if (!launched) { if (vec4) SAGE_CSR_ROW(4, false); else SAGE_CSR_ROW(1, false); }
#undef SAGE_CSR_ROW
    SAGE_CHECK_LAUNCH("csr_row_kernel");
    return SAGE_OK;
}

extern "C" int sage_csr_mean(const int64_t* rowptr, const int32_t* col, int64_t num_nodes, const int32_t* nodes, int32_t n,
                             int64_t max_edges, const float* table, int64_t table_rows, int64_t ld, int32_t dim, int32_t self_loop,
                             const int32_t* any_nonempty, float* out, int64_t ldo, void* workspace, size_t workspace_bytes,
                             sage_stream_t stream) {
    return csr_mean_run("csr_mean", "table_rows", false, rowptr, col, num_nodes, nodes, n, max_edges, nullptr, table, table_rows, ld, dim,
                        self_loop, any_nonempty, out, ldo, workspace, workspace_bytes, stream);
}

extern "C" int sage_csr_mean_indexed(const int64_t* rowptr, const int32_t* col, int64_t num_nodes, const int32_t* nodes, int32_t n,
                                     int64_t max_edges, const int32_t* index, const float* embed, int64_t embed_rows, int64_t ld, int32_t dim,
                                     int32_t self_loop, const int32_t* any_nonempty, float* out, int64_t ldo, void* workspace,
                                     size_t workspace_bytes, sage_stream_t stream) {
    return csr_mean_run("csr_mean_indexed", "embed_rows", true, rowptr, col, num_nodes, nodes, n, max_edges, index, embed, embed_rows, ld, dim,
                        self_loop, any_nonempty, out, ldo, workspace, workspace_bytes, stream);
}

extern "C" int sage_csr_mean_bf16(const int64_t* rowptr, const int32_t* col, int64_t num_nodes, const int32_t* nodes, int32_t n,
                                  int64_t max_edges, const uint16_t* table, int64_t table_rows, int64_t ld, int32_t dim, int32_t self_loop,
                                  const int32_t* any_nonempty, float* out, int64_t ldo, void* workspace, size_t workspace_bytes,
                                  sage_stream_t stream) {
    return csr_mean_run("csr_mean_bf16", "table_rows", false, rowptr, col, num_nodes, nodes, n, max_edges, nullptr, table, table_rows, ld, dim,
                        self_loop, any_nonempty, out, ldo, workspace, workspace_bytes, stream);
}
