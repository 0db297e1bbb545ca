// csr_mean backward for ONE SEED BATCH: the adjoint of sage_csr_mean_indexed(nodes, n, index) -- of sage_csr_mean(nodes, n) without an
// index -- with respect to the table it reads (include/sage355.h).  Seed row r (node v = nodes[r], weight w_r = the forward's 1 / count)
// hands w_r * grad_out[r] to the table row of every entry of row v, and to v's own row if v joined its own mean.  The transposed
// sub-graph that says which seed rows a table row collects from exists for this batch only, so it is built here, per call, the way
// sage_embed_grad.hip builds its own: the TERMS are laid out in a fixed order, sorted by destination row with a stable radix sort, and
// the sorted list is the GROUPED rectangular CSR that sage_csr_mean_backward_grouped takes from its caller.  The sum itself is that
// entry's: bwd_chunk_kernel / bwd_row_kernel of sage_csr_bwd_body.h, the 512-term chunk split of sage_csr_common.h.  No float atomics.
//
// Term order (what fixes the bits of a row): for r = 0 .. n-1 the entries of row nodes[r] in stored order, then nodes[r] itself if it
// joined its own mean.  Position t of a term = tstart[r] + its place in row r's run; the stable sort keeps ascending t inside a key.
//
// Launches, all on the caller's stream, no host round trip:
//   a. count   (self_loop) per seed row its entry count, b. carry, c. start: estart = exclusive scan of the entry counts
//   d. fill + self scan (self_loop): one wave per 512 ENTRIES of the seeds' rows (bwd_self_scan_kernel's cut, over estart instead of
//              the graph's rowptr): found[r] := 1 where row nodes[r] holds nodes[r].  A hub costs what any 512 entries cost.
//   e. count   per seed row w_r and its term count (entries + the self term), f. carry, g. start: tstart, *total_terms
//   h. layout  one wave per 512 term POSITIONS: keys[t] = clamp(index[clamp(id)]) (the forward's clamps), vals[t] = r; positions at or
//              past the terms (or past the capacity) get the sentinel key num_rows
//   i. sort    hipcub::DeviceRadixSort::SortPairs on the bits of num_rows (stable)
//   j. rowptr  rowptr_f[f] = first sorted position whose key is >= f (sorted_rowptr_kernel)
//   1-5.       the family's chunk plan, chunk pass and row pass over (rowptr_f, vals), GROUPED: w and grad_out are indexed by seed row
#include "sage_csr_bwd_body.h"
#include "sage_sorted_terms.h"

namespace {

struct RowsBwdLayout {
    size_t w, found, local, carry, estart, tstart, keys_in, keys_out, vals_in, vals_out, cub, cub_bytes, rowptr_f, total;
    ChunkWs c;
    int64_t slots;       // term positions the workspace holds (at least 1)
    int64_t nblocks;     // count-kernel blocks over the seed rows
};

// The workspace serves either self_loop, so it holds max_edges + n term positions.
bool rows_bwd_layout(int32_t n, int64_t max_edges, int64_t num_rows, int32_t dim, RowsBwdLayout* L) {
    if (n < 0 || max_edges < 0 || num_rows < 0 || num_rows >= (1ll << 31) - 1 || dim < 1 || max_edges + (int64_t)n >= (1ll << 31)) return false;
    L->slots = std::max<int64_t>(max_edges + n, 1);
    L->nblocks = std::max<int64_t>(((int64_t)n + kCountTile - 1) / kCountTile, 1);
    WsCursor cur;
    L->w = cur.take((size_t)n * 4);
    L->found = cur.take((size_t)n * 4);
    L->local = cur.take((size_t)n * 8);
    L->carry = cur.take((size_t)(L->nblocks + 1) * 8);
    L->estart = cur.take((size_t)(n + 1) * 8);
    L->tstart = cur.take((size_t)(n + 1) * 8);
    L->keys_in = cur.take((size_t)L->slots * 4);
    L->keys_out = cur.take((size_t)L->slots * 4);
    L->vals_in = cur.take((size_t)L->slots * 4);
    L->vals_out = cur.take((size_t)L->slots * 4);
    L->cub_bytes = sort_temp_reserve(L->slots);
    L->cub = cur.take(L->cub_bytes);
    L->rowptr_f = cur.take((size_t)(num_rows + 1) * 8);
    if (!chunk_ws(num_rows, L->slots, dim, cur, &L->c)) return false;      // every long run's chunks fit: at most slots terms in all
    L->total = cur.off;
    return true;
}

// a / e. count_block_scan (sage_csr_common.h) over the seed rows, of their ENTRY counts (TERMS false) or their TERM counts (TERMS
// true: the self term joins where found[r] == 0, and w[r] := the forward's 1 / count): local[r] := block-local exclusive offset,
// carry[block] := the block's sum
template <bool TERMS>
__global__ __launch_bounds__(kCountThreads) void rows_count_kernel(const int64_t* __restrict__ rowptr, int64_t num_nodes,
                                                                    const int32_t* __restrict__ nodes, int n, int self_loop,
                                                                    const int32_t* __restrict__ found, float* __restrict__ w,
                                                                    int64_t* __restrict__ local, int64_t* __restrict__ carry) {
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
            c[i] = e - b;
            if constexpr (TERMS) {
                if (self_loop && v >= 0 && found[r0 + i] == 0) c[i] += 1;      // a node outside the graph: an empty row without a self term
                w[r0 + i] = c[i] > 0 ? 1.0f / (float)c[i] : 0.f;
            }
        }
    }
    count_block_scan(c, r0, n, local, carry);
}

// c / g. start[r] := the global exclusive offset, start[n] := the total (also to *total_out when given)
__global__ __launch_bounds__(256) void rows_start_kernel(const int64_t* __restrict__ local, const int64_t* __restrict__ carry, int nb, int n,
                                                         int64_t* __restrict__ start, int64_t* __restrict__ total_out) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r < n) start[r] = local[r] + carry[r / kCountTile];
    if (r == n) {
        start[n] = carry[nb];
        if (total_out) *total_out = carry[nb];
    }
}

// d. found[r] := 1 for every seed row r whose node is an entry of its own row.  Entry position p of the batch is entry p - estart[r]
// of row r = the last row that starts at or before p (an empty row shares its start with the next row and is never that one).
__global__ __launch_bounds__(256) void rows_self_scan_kernel(const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                             int64_t num_nodes, const int32_t* __restrict__ nodes, int n,
                                                             const int64_t* __restrict__ estart, int32_t* __restrict__ found) {
    const int lane = sage_lane();
    const int64_t wave = (int64_t)((blockIdx.x * blockDim.x + threadIdx.x) >> 6);
    const int64_t nwaves = (int64_t)((gridDim.x * blockDim.x) >> 6);
    const int64_t total = rowptr[num_nodes];
    const int64_t entries = estart[n];
    for (int64_t s0 = wave * kChunk; s0 < entries; s0 += nwaves * kChunk) {
        const int64_t s1 = min(s0 + kChunk, entries);
        const int32_t r_lo = __builtin_amdgcn_readfirstlane(row_of(estart, 0, n - 1, s0));
        const int32_t r_hi = __builtin_amdgcn_readfirstlane(row_of(estart, r_lo, n - 1, s1 - 1));
        for (int64_t p = s0 + lane; p < s1; p += kWave) {
            const int32_t r = row_of(estart, r_lo, r_hi, p);
            int32_t v;
            int64_t b, e;
            row_span(rowptr, num_nodes, nodes, r, total, v, b, e);
            const int64_t j = p - estart[r];
            if (j >= 0 && j < e - b && col[b + j] == v) found[r] = 1;      // racing stores all store 1
        }
    }
}

// h. keys / vals of every term position below `slots`: live positions (below the term count and the capacity) name their table row
// and their seed row, the others hold the sentinel.
__global__ __launch_bounds__(256) void rows_layout_kernel(const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                          int64_t num_nodes, const int32_t* __restrict__ nodes, int n,
                                                          const int64_t* __restrict__ tstart, const int32_t* __restrict__ index, int num_rows,
                                                          int64_t slots, int64_t capacity, int32_t* __restrict__ keys,
                                                          int32_t* __restrict__ vals) {
    const int lane = sage_lane();
    const int64_t wave = (int64_t)((blockIdx.x * blockDim.x + threadIdx.x) >> 6);
    const int64_t nwaves = (int64_t)((gridDim.x * blockDim.x) >> 6);
    const int64_t total = rowptr[num_nodes];
    const int64_t live = min(tstart[n], capacity);                  // terms at positions past the capacity are dropped
    const int last_node = (int)num_nodes - 1;
    for (int64_t s0 = wave * kChunk; s0 < slots; s0 += nwaves * kChunk) {
        const int64_t s1 = min(s0 + kChunk, slots);
        int32_t r_lo = 0, r_hi = 0;
        if (s0 < live) {
            r_lo = __builtin_amdgcn_readfirstlane(row_of(tstart, 0, n - 1, s0));
            r_hi = __builtin_amdgcn_readfirstlane(row_of(tstart, r_lo, n - 1, min(s1, live) - 1));
        }
        for (int64_t p = s0 + lane; p < s1; p += kWave) {
            int key = num_rows, val = 0;
            if (p < live) {
                const int32_t r = row_of(tstart, r_lo, r_hi, p);
                int32_t v;
                int64_t b, e;
                row_span(rowptr, num_nodes, nodes, r, total, v, b, e);
                const int64_t j = p - tstart[r];
                if (v >= 0 && j >= 0 && j <= e - b) {               // j == e - b: the self term
                    const int id = j < e - b ? col[b + j] : v;
                    const int row = index ? index[min(max(id, 0), last_node)] : id;       // the forward's clamps: node id, then row
                    key = min(max(row, 0), num_rows - 1);
                    val = r;
                }
            }
            keys[p] = key;
            vals[p] = val;
        }
    }
}

}  // namespace

extern "C" size_t sage_csr_mean_backward_rows_workspace_bytes(int32_t n, int64_t max_edges, int64_t num_rows, int32_t dim) {
    RowsBwdLayout L;
    return rows_bwd_layout(n, max_edges, num_rows, dim, &L) ? L.total : 0;
}

extern "C" int sage_csr_mean_backward_rows(const int64_t* rowptr, const int32_t* col, int64_t num_nodes, const int32_t* nodes, int32_t n,
                                           int64_t max_edges, const int32_t* index, int64_t num_rows, const float* grad_out, int64_t ldg,
                                           int32_t dim, int32_t self_loop, float* grad_table, int64_t ldgt, int64_t* total_terms,
                                           void* workspace, size_t workspace_bytes, sage_stream_t stream) {
    // shapes first, then pointers, then the workspace: sage_csr_mean_backward's order
    SAGE_REQUIRE(num_nodes >= 0 && num_nodes < (1ll << 31), "csr_mean_backward_rows: num_nodes = %lld", (long long)num_nodes);
    SAGE_REQUIRE(n >= 0, "csr_mean_backward_rows: n = %d", n);
    SAGE_REQUIRE(max_edges >= 0, "csr_mean_backward_rows: max_edges = %lld", (long long)max_edges);
    SAGE_REQUIRE(num_rows >= 0 && num_rows < (1ll << 31) - 1, "csr_mean_backward_rows: num_rows = %lld", (long long)num_rows);
    SAGE_REQUIRE(num_rows > 0 || n == 0, "csr_mean_backward_rows: num_rows = 0 with n = %d seed rows", n);
    SAGE_REQUIRE(dim >= 1 && ldg >= dim && ldgt >= dim, "csr_mean_backward_rows: dim = %d, ldg = %lld, ldgt = %lld", dim, (long long)ldg,
                 (long long)ldgt);
    SAGE_REQUIRE(self_loop == 0 || self_loop == 1, "csr_mean_backward_rows: self_loop = %d", self_loop);
    SAGE_REQUIRE(rowptr && col && nodes && grad_out && grad_table, "csr_mean_backward_rows: NULL array");
    RowsBwdLayout L;
    SAGE_REQUIRE(rows_bwd_layout(n, max_edges, num_rows, dim, &L),
                 "csr_mean_backward_rows: n = %d, max_edges = %lld, num_rows = %lld, dim = %d out of range (max_edges + n < 2^31)", n,
                 (long long)max_edges, (long long)num_rows, dim);
    if (const int rc = csr_workspace_check("csr_mean_backward_rows", workspace, workspace_bytes, L.total)) return rc;
    if (num_rows == 0) return SAGE_OK;

    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace;
    float* w = (float*)(ws + L.w);
    int32_t* found = (int32_t*)(ws + L.found);
    int64_t* local = (int64_t*)(ws + L.local);
    int64_t* carry = (int64_t*)(ws + L.carry);
    int64_t* estart = (int64_t*)(ws + L.estart);
    int64_t* tstart = (int64_t*)(ws + L.tstart);
    int32_t* keys_in = (int32_t*)(ws + L.keys_in);
    int32_t* keys_out = (int32_t*)(ws + L.keys_out);
    int32_t* vals_in = (int32_t*)(ws + L.vals_in);
    int32_t* vals_out = (int32_t*)(ws + L.vals_out);
    int64_t* rowptr_f = (int64_t*)(ws + L.rowptr_f);
    const int R = (int)num_rows;
    const BwdSum sum{rowptr_f, vals_out, num_rows, true, nullptr, R, w, nullptr, n, grad_out, ldg, dim, grad_table, ldgt};

    if (n == 0) {                                        // no term: every row of grad_table is stored as zeros
        if (const int rc = sage_fill_u32(rowptr_f, 0u, (size_t)(num_rows + 1) * 2, st)) return rc;
        if (total_terms)
            if (const int rc = sage_fill_u32(total_terms, 0u, 2, st)) return rc;
        return bwd_sum_launch(sum, workspace, L.c, st);
    }

    const int64_t capacity = max_edges + (self_loop ? n : 0);
    const int64_t slots = std::max<int64_t>(capacity, 1);         // <= L.slots
    const int bits = sort_key_bits(num_rows);
    size_t sort_bytes = 0;
    if (sort_temp_bytes((int)slots, bits, &sort_bytes) != hipSuccess || sort_bytes > L.cub_bytes) {
        sage_set_error("csr_mean_backward_rows: the radix sort asks for %zu bytes of temporary, %zu reserved", sort_bytes, L.cub_bytes);
        return SAGE_ELAUNCH;
    }

    const int nb = (int)L.nblocks;
    const int entry_blocks = (int)std::min<int64_t>(std::max<int64_t>((max_edges / kChunk + 4) / 4, 1), kNumCU * 8);
    if (self_loop) {
        hipLaunchKernelGGL(rows_count_kernel<false>, dim3(nb), dim3(kCountThreads), 0, st, rowptr, num_nodes, nodes, n, 0, (const int32_t*)nullptr,
                           (float*)nullptr, local, carry);
        SAGE_CHECK_LAUNCH("rows_count_kernel (entries)");
        hipLaunchKernelGGL(csr_carry_kernel, dim3(1), dim3(kCarryThreads), 0, st, carry, nb);
        SAGE_CHECK_LAUNCH("csr_carry_kernel (entries)");
        hipLaunchKernelGGL(rows_start_kernel, dim3(sage_cdiv((int64_t)n + 1, 256)), dim3(256), 0, st, (const int64_t*)local, (const int64_t*)carry, nb,
                           n, estart, (int64_t*)nullptr);
        SAGE_CHECK_LAUNCH("rows_start_kernel (entries)");
        if (const int rc = sage_fill_u32(found, 0u, (size_t)n, st)) return rc;
        hipLaunchKernelGGL(rows_self_scan_kernel, dim3(entry_blocks), dim3(256), 0, st, rowptr, col, num_nodes, nodes, n, (const int64_t*)estart,
                           found);
        SAGE_CHECK_LAUNCH("rows_self_scan_kernel");
    }
    hipLaunchKernelGGL(rows_count_kernel<true>, dim3(nb), dim3(kCountThreads), 0, st, rowptr, num_nodes, nodes, n, (int)self_loop,
                       (const int32_t*)found, w, local, carry);
    SAGE_CHECK_LAUNCH("rows_count_kernel (terms)");
    hipLaunchKernelGGL(csr_carry_kernel, dim3(1), dim3(kCarryThreads), 0, st, carry, nb);
    SAGE_CHECK_LAUNCH("csr_carry_kernel (terms)");
    hipLaunchKernelGGL(rows_start_kernel, dim3(sage_cdiv((int64_t)n + 1, 256)), dim3(256), 0, st, (const int64_t*)local, (const int64_t*)carry, nb, n,
                       tstart, total_terms);
    SAGE_CHECK_LAUNCH("rows_start_kernel (terms)");

    const int term_blocks = (int)std::min<int64_t>(std::max<int64_t>((slots / kChunk + 4) / 4, 1), kNumCU * 8);
    hipLaunchKernelGGL(rows_layout_kernel, dim3(term_blocks), dim3(256), 0, st, rowptr, col, num_nodes, nodes, n, (const int64_t*)tstart, index, R,
                       slots, capacity, keys_in, vals_in);
    SAGE_CHECK_LAUNCH("rows_layout_kernel");
    size_t cub_bytes = L.cub_bytes;
    if (hipcub::DeviceRadixSort::SortPairs(ws + L.cub, cub_bytes, (const int32_t*)keys_in, keys_out, (const int32_t*)vals_in, vals_out, (int)slots, 0,
                                           bits, st) != hipSuccess) {
        sage_set_error("csr_mean_backward_rows: radix sort failed");
        return SAGE_ELAUNCH;
    }
    hipLaunchKernelGGL(sorted_rowptr_kernel, dim3(sage_cdiv(num_rows + 1, 256)), dim3(256), 0, st, (const int32_t*)keys_out, (int)slots, R, rowptr_f);
    SAGE_CHECK_LAUNCH("sorted_rowptr_kernel");
    return bwd_sum_launch(sum, workspace, L.c, st);
}
