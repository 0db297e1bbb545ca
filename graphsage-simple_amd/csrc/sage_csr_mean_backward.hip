// csr_mean backward: the adjoint of sage_csr_mean(nodes = NULL, n = num_nodes) with respect to `table` (include/sage355.h).
//
// The forward's row v is (1 / c_v) * (sum of table rows of v's entries [+ table[v] by the set-union rule]); so table row u
// receives w_x * grad_out[x] once per entry u of row x, plus w_u * grad_out[u] if u joined its own mean.  The entries that
// name u are row u of the TRANSPOSED CSR, which the caller builds once per graph: the sum is then the forward's computation on
// the transposed graph -- same split of long rows into chunks of SAGE_CSR_MEAN_CHUNK entries, same launches, same fall-back
// when the item list is too small -- with a weight per entry and no final division.  No float atomics.
//
// Launches, all on the caller's stream, no host round trip:
//   a. fill     found[v] := 0                                             (self_loop only)
//   b. scan     one wave per 512 entries of the FORWARD col[]: found[v] := 1 where row v holds v.  Cut by entries, not by
//               rows, so a hub costs its chunks' waves what any other 512 entries cost; the row of an entry is found by a
//               bisection of rowptr inside the rows the wave's 512 entries span.  Racing stores all store 1.   (self_loop only)
//   c. weight   per node: flag[v] := extra_v (in place of found), w[v] := c_v > 0 ? 1.0f / (float)c_v : 0
//   1-3. count, carry, expand on the transposed rows (sage_csr_common.h: csr_chunk_plan)
//   4. chunk    one wave per item: partials[item] := the chunk's weighted sum
//   5. rows     one wave per row: short rows summed in place; long rows = their partials in chunk order; self term; store
//
// Arithmetic of a row (its bits depend on nothing else): p_c = fma(w_x, g_x, ...fma(w_x0, g_x0, 0)) over chunk c's entries in
// stored order; S = 0 + p_0 + p_1 + ...; S = fma(w_u, g_u, S) if extra_u; grad_table[r] = S.  Every term is ONE fma, in the
// chunk pass and in the fall-back alike: sum_weighted is the only place that forms a term, and sage_csr_common.h's chunked_row_sum
// the only place that adds a row's terms and partials up (with its item check, chunk_item, shared by the files of this family).
// sum_weighted and the kernels of launches 4 and 5 live in sage_csr_bwd_body.h: sage_csr_mean_backward_rows.hip runs them too.
//
// GROUPED instantiations (sage_csr_mean_backward_grouped): the gradient of an embedding read as embed[index[v]] through the
// forward.  The caller's rectangular CSR has one row per EMBEDDING row and lists, for every node that reads it, that node's
// transposed entries and then the node itself if it joined its own mean.  So the row count (groups) is separate from the source
// count (nodes) that clamps ids into grad_out and w, and the row kernel's own self term is off: the self entries are in the list.
#include "sage_csr_bwd_body.h"

namespace {

struct BwdLayout {
    ChunkWs c;
    size_t weight, flag, total;
};

bool bwd_layout(int64_t num_nodes, int32_t n, int64_t max_edges, int32_t dim, BwdLayout* L) {
    if (num_nodes < 0 || num_nodes >= (1ll << 31) || n < 0 || max_edges < 0 || dim < 1) return false;
    WsCursor cur;
    if (!chunk_ws(n, max_edges, dim, cur, &L->c)) return false;
    L->weight = cur.take((size_t)num_nodes * 4);
    L->flag = cur.take((size_t)num_nodes * 4);
    L->total = cur.off;
    return true;
}

// b. found[v] := 1 for every node v that is an entry of its own forward row
__global__ __launch_bounds__(256) void bwd_self_scan_kernel(const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                            int64_t num_nodes, int32_t* __restrict__ found) {
    const int lane = sage_lane();
    const int64_t wave = (int64_t)((blockIdx.x * blockDim.x + threadIdx.x) >> 6);
    const int64_t nwaves = (int64_t)((gridDim.x * blockDim.x) >> 6);
    const int64_t total = rowptr[num_nodes];
    const int32_t last = (int32_t)num_nodes - 1;
    for (int64_t s0 = wave * kChunk; s0 < total; s0 += nwaves * kChunk) {
        const int64_t s1 = min(s0 + kChunk, total);
        const int32_t r_lo = __builtin_amdgcn_readfirstlane(row_of(rowptr, 0, last, s0));
        const int32_t r_hi = __builtin_amdgcn_readfirstlane(row_of(rowptr, r_lo, last, s1 - 1));
        for (int64_t e = s0 + lane; e < s1; e += kWave) {
            const int32_t r = row_of(rowptr, r_lo, r_hi, e);
            if (col[e] == r) found[r] = 1;
        }
    }
}

// c. flag[v] := extra_v (it held found[v]; not read without self_loop), w[v] := the forward's 1 / count
__global__ __launch_bounds__(256) void bwd_weight_kernel(const int64_t* __restrict__ rowptr, int64_t num_nodes, int self_loop,
                                                         int32_t* __restrict__ flag, float* __restrict__ w) {
    const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= num_nodes) return;
    const int64_t total = rowptr[num_nodes];
    int32_t node;
    int64_t b, e;
    row_span(rowptr, num_nodes, nullptr, (int)v, total, node, b, e);
    const int extra = (self_loop && flag[v] == 0) ? 1 : 0;
    const int64_t c = (e - b) + extra;
    flag[v] = extra;
    w[v] = c > 0 ? 1.0f / (float)c : 0.f;
}

}  // namespace

extern "C" size_t sage_csr_mean_backward_workspace_bytes(int64_t num_nodes, int32_t n, int64_t max_edges, int32_t dim) {
    BwdLayout L;
    return bwd_layout(num_nodes, n, max_edges, dim, &L) ? L.total : 0;
}

// Launches a-c on the forward CSR, then 1-5 on the rows of (rowptr_t, col_t): the num_nodes transposed rows, or with `grouped` the
// num_rows rows of the grouped list.  Arguments are validated by the entries.
static int bwd_launch(const int64_t* rowptr, const int32_t* col, const int64_t* rowptr_t, const int32_t* col_t, int64_t num_nodes,
                      int64_t num_rows, bool grouped, const int32_t* nodes, int32_t n, int64_t max_edges, const float* grad_out, int64_t ldg,
                      int32_t dim, int32_t self_loop, float* grad_table, int64_t ldgt, void* workspace, const BwdLayout& L,
                      sage_stream_t stream) {
    hipStream_t st = (hipStream_t)stream;
    float* w = (float*)((char*)workspace + L.weight);
    int32_t* flag = (int32_t*)((char*)workspace + L.flag);

    // the weights of the forward's rows.  num_nodes >= 1 here: n > 0 rows without a node list need it, and with one and no nodes
    // every row is empty -- the kernels below then read neither w nor flag
    if (num_nodes > 0) {
        if (self_loop) {
            const int rc = sage_fill_u32(flag, 0u, (size_t)num_nodes, st);
            if (rc != SAGE_OK) return rc;
            const int blocks = (int)std::min<int64_t>(std::max<int64_t>((max_edges / kChunk + 4) / 4, 1), kNumCU * 8);
            hipLaunchKernelGGL(bwd_self_scan_kernel, dim3(blocks), dim3(256), 0, st, rowptr, col, num_nodes, flag);
            SAGE_CHECK_LAUNCH("bwd_self_scan_kernel");
        }
        hipLaunchKernelGGL(bwd_weight_kernel, dim3(sage_cdiv(num_nodes, 256)), dim3(256), 0, st, rowptr, num_nodes, (int)self_loop, flag, w);
        SAGE_CHECK_LAUNCH("bwd_weight_kernel");
    }

    return bwd_sum_launch(BwdSum{rowptr_t, col_t, num_rows, grouped, nodes, n, w, flag, num_nodes, grad_out, ldg, dim, grad_table, ldgt}, workspace,
                          L.c, st);
}

extern "C" int sage_csr_mean_backward(const int64_t* rowptr, const int32_t* col, const int64_t* rowptr_t, const int32_t* col_t,
                                      int64_t num_nodes, const int32_t* nodes, int32_t n, int64_t max_edges, const float* grad_out,
                                      int64_t ldg, int32_t dim, int32_t self_loop, float* grad_table, int64_t ldgt, void* workspace,
                                      size_t workspace_bytes, sage_stream_t stream) {
    // shapes first, then pointers: a bad shape is reported as such whatever the pointers are
    SAGE_REQUIRE(num_nodes >= 0 && num_nodes < (1ll << 31), "csr_mean_backward: num_nodes = %lld", (long long)num_nodes);
    SAGE_REQUIRE(n >= 0 && (nodes || n <= num_nodes), "csr_mean_backward: n = %d rows for %lld nodes without a node list", n,
                 (long long)num_nodes);
    SAGE_REQUIRE(max_edges >= 0, "csr_mean_backward: max_edges = %lld", (long long)max_edges);
    SAGE_REQUIRE(dim >= 1 && ldg >= dim && ldgt >= dim, "csr_mean_backward: dim = %d, ldg = %lld, ldgt = %lld", dim, (long long)ldg,
                 (long long)ldgt);
    SAGE_REQUIRE(self_loop == 0 || self_loop == 1, "csr_mean_backward: self_loop = %d", self_loop);
    SAGE_REQUIRE(rowptr && col && rowptr_t && col_t && grad_out && grad_table, "csr_mean_backward: NULL array");
    BwdLayout L;
    SAGE_REQUIRE(bwd_layout(num_nodes, n, max_edges, dim, &L), "csr_mean_backward: n = %d, max_edges = %lld, dim = %d out of range", n,
                 (long long)max_edges, dim);
    if (const int rc = csr_workspace_check("csr_mean_backward", workspace, workspace_bytes, L.total)) return rc;
    if (n == 0) return SAGE_OK;
    return bwd_launch(rowptr, col, rowptr_t, col_t, num_nodes, num_nodes, false, nodes, n, max_edges, grad_out, ldg, dim, self_loop, grad_table,
                      ldgt, workspace, L, stream);
}

extern "C" size_t sage_csr_mean_backward_grouped_workspace_bytes(int64_t num_nodes, int64_t num_groups, int64_t max_edges, int32_t dim) {
    BwdLayout L;
    if (num_groups < 0 || num_groups >= (1ll << 31)) return 0;
    return bwd_layout(num_nodes, (int32_t)num_groups, max_edges, dim, &L) ? L.total : 0;
}

extern "C" int sage_csr_mean_backward_grouped(const int64_t* rowptr, const int32_t* col, const int64_t* rowptr_gt, const int32_t* col_gt,
                                              int64_t num_nodes, int64_t num_groups, int64_t max_edges, const float* grad_out, int64_t ldg,
                                              int32_t dim, int32_t self_loop, float* grad_embed, int64_t ldge, void* workspace,
                                              size_t workspace_bytes, sage_stream_t stream) {
    // shapes first, then pointers, then the workspace: sage_csr_mean_backward's order
    SAGE_REQUIRE(num_nodes >= 0 && num_nodes < (1ll << 31), "csr_mean_backward_grouped: num_nodes = %lld", (long long)num_nodes);
    SAGE_REQUIRE(num_groups >= 0 && num_groups < (1ll << 31), "csr_mean_backward_grouped: num_groups = %lld", (long long)num_groups);
    SAGE_REQUIRE(num_groups == 0 || num_nodes >= 1, "csr_mean_backward_grouped: num_nodes = 0 with %lld groups", (long long)num_groups);
    SAGE_REQUIRE(max_edges >= 0, "csr_mean_backward_grouped: max_edges = %lld", (long long)max_edges);
    SAGE_REQUIRE(dim >= 1 && ldg >= dim && ldge >= dim, "csr_mean_backward_grouped: dim = %d, ldg = %lld, ldge = %lld", dim, (long long)ldg,
                 (long long)ldge);
    SAGE_REQUIRE(self_loop == 0 || self_loop == 1, "csr_mean_backward_grouped: self_loop = %d", self_loop);
    SAGE_REQUIRE(rowptr && col && rowptr_gt && col_gt && grad_out && grad_embed, "csr_mean_backward_grouped: NULL array");
    BwdLayout L;
    SAGE_REQUIRE(bwd_layout(num_nodes, (int32_t)num_groups, max_edges, dim, &L),
                 "csr_mean_backward_grouped: num_groups = %lld, max_edges = %lld, dim = %d out of range", (long long)num_groups,
                 (long long)max_edges, dim);
    if (const int rc = csr_workspace_check("csr_mean_backward_grouped", workspace, workspace_bytes, L.total)) return rc;
    if (num_groups == 0) return SAGE_OK;
    return bwd_launch(rowptr, col, rowptr_gt, col_gt, num_nodes, num_groups, true, nullptr, (int32_t)num_groups, max_edges, grad_out, ldg, dim,
                      self_loop, grad_embed, ldge, workspace, L, stream);
}
