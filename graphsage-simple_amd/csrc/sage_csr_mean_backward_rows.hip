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
// sage_csr_mean_backward_touched (below) is the same sum for the table rows that have a term only, with the SGD update of those rows
// fused in: steps a-i are one function behind both entries (rows_sort_terms), step j is sage_sorted_terms.h's run list of the sorted
// keys instead of a row pointer over the table, the chunk plan and chunk pass walk the runs, and bwd_runs_row_kernel strides over the
// runs u < U, U read on the device.  Nothing there is sized by num_rows.
#include "sage_csr_bwd_body.h"
#include "sage_sorted_terms.h"

namespace {

// What steps a-i of both entries need of a workspace.  It serves either self_loop, so it holds max_edges + n term positions.
struct TermsWs {
    size_t w, found, local, carry, estart, tstart;
    SortPairsWs pairs;
    int64_t slots;       // term positions the workspace holds (at least 1)
    int64_t nblocks;     // count-kernel blocks over the seed rows
};

bool terms_ws(int32_t n, int64_t max_edges, int64_t num_rows, int32_t dim, WsCursor& cur, TermsWs* T) {
    if (n < 0 || max_edges < 0 || num_rows < 0 || num_rows >= (1ll << 31) - 1 || dim < 1 || max_edges + (int64_t)n >= (1ll << 31)) return false;
    T->slots = std::max<int64_t>(max_edges + n, 1);
    T->nblocks = std::max<int64_t>(((int64_t)n + kCountTile - 1) / kCountTile, 1);
    T->w = cur.take((size_t)n * 4);
    T->found = cur.take((size_t)n * 4);
    T->local = cur.take((size_t)n * 8);
    T->carry = cur.take((size_t)(T->nblocks + 1) * 8);
    T->estart = cur.take((size_t)(n + 1) * 8);
    T->tstart = cur.take((size_t)(n + 1) * 8);
    T->pairs.take(T->slots, cur);
    return true;
}

struct RowsBwdLayout {
    TermsWs t;
    size_t rowptr_f, total;
    ChunkWs c;
};

bool rows_bwd_layout(int32_t n, int64_t max_edges, int64_t num_rows, int32_t dim, RowsBwdLayout* L) {
    WsCursor cur;
    if (!terms_ws(n, max_edges, num_rows, dim, cur, &L->t)) return false;
    L->rowptr_f = cur.take((size_t)(num_rows + 1) * 8);
    if (!chunk_ws(num_rows, L->t.slots, dim, cur, &L->c)) return false;      // every long run's chunks fit: at most slots terms in all
    L->total = cur.off;
    return true;
}

// sage_csr_mean_backward_touched: a run list of at most runs_cap = min(max_edges + n, num_rows) runs instead of rowptr_f; for
// num_rows >= max_edges + n nothing here depends on num_rows.
struct TouchedLayout {
    TermsWs t;
    RunListWs r;
    size_t total;
    ChunkWs c;
};

bool touched_layout(int32_t n, int64_t max_edges, int64_t num_rows, int32_t dim, TouchedLayout* L) {
    WsCursor cur;
    if (!terms_ws(n, max_edges, num_rows, dim, cur, &L->t)) return false;
    L->r.take(L->t.slots, std::min<int64_t>(max_edges + n, num_rows), cur);   // distinct rows with a term: what every array below is sized by
    if (!chunk_ws(L->r.runs_cap, L->t.slots, dim, cur, &L->c)) return false;
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

// The sorted terms: keys ascending (table rows, then the sentinels num_rows), vals the seed row of each term, w the weight of each
// seed row; `slots` positions in all.
struct SortedTerms {
    const int32_t* keys;
    const int32_t* vals;
    const float* w;
    int64_t slots;
};

// What both entries pass on to steps a-i.
struct TermsArgs {
    const int64_t* rowptr; const int32_t* col; int64_t num_nodes;
    const int32_t* nodes; int32_t n; int64_t max_edges;
    const int32_t* index; int64_t num_rows; int32_t self_loop;
    int64_t* total_terms;
};

// Steps a-i of both entries (n >= 1, num_rows >= 1), errors under the entry's `name`: the sort's temporary is checked before anything
// is launched.
int rows_sort_terms(const char* name, const TermsArgs& a, void* workspace, const TermsWs& L, hipStream_t st, SortedTerms* T) {
    char* ws = (char*)workspace;
    float* w = (float*)(ws + L.w);
    int32_t* found = (int32_t*)(ws + L.found);
    int64_t* local = (int64_t*)(ws + L.local);
    int64_t* carry = (int64_t*)(ws + L.carry);
    int64_t* estart = (int64_t*)(ws + L.estart);
    int64_t* tstart = (int64_t*)(ws + L.tstart);
    const int n = a.n, R = (int)a.num_rows;
    const int64_t capacity = a.max_edges + (a.self_loop ? n : 0);
    const int64_t slots = std::max<int64_t>(capacity, 1);         // <= L.slots
    const int bits = sort_key_bits(a.num_rows);
    if (const int rc = sort_temp_check(name, (int)slots, bits, L.pairs)) return rc;

    const int nb = (int)L.nblocks;
    const int entry_blocks = (int)std::min<int64_t>(std::max<int64_t>((a.max_edges / kChunk + 4) / 4, 1), kNumCU * 8);
    if (a.self_loop) {
        hipLaunchKernelGGL(rows_count_kernel<false>, dim3(nb), dim3(kCountThreads), 0, st, a.rowptr, a.num_nodes, a.nodes, n, 0,
                           (const int32_t*)nullptr, (float*)nullptr, local, carry);
        SAGE_CHECK_LAUNCH("rows_count_kernel (entries)");
        hipLaunchKernelGGL(csr_carry_kernel, dim3(1), dim3(kCarryThreads), 0, st, carry, nb);
        SAGE_CHECK_LAUNCH("csr_carry_kernel (entries)");
        hipLaunchKernelGGL(rows_start_kernel, dim3(sage_cdiv((int64_t)n + 1, 256)), dim3(256), 0, st, (const int64_t*)local, (const int64_t*)carry, nb,
                           n, estart, (int64_t*)nullptr);
        SAGE_CHECK_LAUNCH("rows_start_kernel (entries)");
        if (const int rc = sage_fill_u32(found, 0u, (size_t)n, st)) return rc;
        hipLaunchKernelGGL(rows_self_scan_kernel, dim3(entry_blocks), dim3(256), 0, st, a.rowptr, a.col, a.num_nodes, a.nodes, n,
                           (const int64_t*)estart, found);
        SAGE_CHECK_LAUNCH("rows_self_scan_kernel");
    }
    hipLaunchKernelGGL(rows_count_kernel<true>, dim3(nb), dim3(kCountThreads), 0, st, a.rowptr, a.num_nodes, a.nodes, n, (int)a.self_loop,
                       (const int32_t*)found, w, local, carry);
    SAGE_CHECK_LAUNCH("rows_count_kernel (terms)");
    hipLaunchKernelGGL(csr_carry_kernel, dim3(1), dim3(kCarryThreads), 0, st, carry, nb);
    SAGE_CHECK_LAUNCH("csr_carry_kernel (terms)");
    hipLaunchKernelGGL(rows_start_kernel, dim3(sage_cdiv((int64_t)n + 1, 256)), dim3(256), 0, st, (const int64_t*)local, (const int64_t*)carry, nb, n,
                       tstart, a.total_terms);
    SAGE_CHECK_LAUNCH("rows_start_kernel (terms)");

    const int term_blocks = (int)std::min<int64_t>(std::max<int64_t>((slots / kChunk + 4) / 4, 1), kNumCU * 8);
    hipLaunchKernelGGL(rows_layout_kernel, dim3(term_blocks), dim3(256), 0, st, a.rowptr, a.col, a.num_nodes, a.nodes, n, (const int64_t*)tstart,
                       a.index, R, slots, capacity, L.pairs.keys(ws), L.pairs.vals(ws));
    SAGE_CHECK_LAUNCH("rows_layout_kernel");
    if (const int rc = sort_pairs(name, ws, L.pairs, (int)slots, bits, st)) return rc;
    *T = SortedTerms{L.pairs.sorted_keys(ws), L.pairs.sorted_vals(ws), w, slots};
    return SAGE_OK;
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
    int64_t* rowptr_f = (int64_t*)((char*)workspace + L.rowptr_f);
    const int R = (int)num_rows;

    if (n == 0) {                                        // no term: every row of grad_table is stored as zeros
        char* ws = (char*)workspace;
        const BwdSum sum{rowptr_f, L.t.pairs.sorted_vals(ws), num_rows, true, nullptr, R, (const float*)(ws + L.t.w), nullptr, n, grad_out, ldg, dim,
                         grad_table, ldgt};
        if (const int rc = sage_fill_u32(rowptr_f, 0u, (size_t)(num_rows + 1) * 2, st)) return rc;
        if (total_terms)
            if (const int rc = sage_fill_u32(total_terms, 0u, 2, st)) return rc;
        return bwd_sum_launch(sum, workspace, L.c, st);
    }

    SortedTerms T;
    const TermsArgs args{rowptr, col, num_nodes, nodes, n, max_edges, index, num_rows, self_loop, total_terms};
    if (const int rc = rows_sort_terms("csr_mean_backward_rows", args, workspace, L.t, st, &T)) return rc;
    hipLaunchKernelGGL(sorted_rowptr_kernel, dim3(sage_cdiv(num_rows + 1, 256)), dim3(256), 0, st, T.keys, (int)T.slots, R, rowptr_f);
    SAGE_CHECK_LAUNCH("sorted_rowptr_kernel");
    const BwdSum sum{rowptr_f, T.vals, num_rows, true, nullptr, R, T.w, nullptr, n, grad_out, ldg, dim, grad_table, ldgt};
    return bwd_sum_launch(sum, workspace, L.c, st);
}

extern "C" size_t sage_csr_mean_backward_touched_workspace_bytes(int32_t n, int64_t max_edges, int64_t num_rows, int32_t dim) {
    TouchedLayout L;
    return touched_layout(n, max_edges, num_rows, dim, &L) ? L.total : 0;
}

extern "C" int sage_csr_mean_backward_touched(const int64_t* rowptr, const int32_t* col, int64_t num_nodes, const int32_t* nodes, int32_t n,
                                              int64_t max_edges, const int32_t* index, int64_t num_rows, const float* grad_out, int64_t ldg,
                                              int32_t dim, int32_t self_loop, int32_t* num_rows_out, int32_t* rows_out, float* grad_rows,
                                              int64_t max_rows, int64_t ldr, float* table, int64_t ldt, float lr, int64_t* total_terms,
                                              void* workspace, size_t workspace_bytes, sage_stream_t stream) {
    // sage_csr_mean_backward_rows' rules and order: shapes first, then pointers, then the workspace
    SAGE_REQUIRE(num_nodes >= 0 && num_nodes < (1ll << 31), "csr_mean_backward_touched: num_nodes = %lld", (long long)num_nodes);
    SAGE_REQUIRE(n >= 0, "csr_mean_backward_touched: n = %d", n);
    SAGE_REQUIRE(max_edges >= 0, "csr_mean_backward_touched: max_edges = %lld", (long long)max_edges);
    SAGE_REQUIRE(num_rows >= 0 && num_rows < (1ll << 31) - 1, "csr_mean_backward_touched: num_rows = %lld", (long long)num_rows);
    SAGE_REQUIRE(num_rows > 0 || n == 0, "csr_mean_backward_touched: num_rows = 0 with n = %d seed rows", n);
    SAGE_REQUIRE(dim >= 1 && ldg >= dim, "csr_mean_backward_touched: dim = %d, ldg = %lld", dim, (long long)ldg);
    SAGE_REQUIRE(!grad_rows || ldr >= dim, "csr_mean_backward_touched: dim = %d, ldr = %lld", dim, (long long)ldr);
    SAGE_REQUIRE(!table || ldt >= dim, "csr_mean_backward_touched: dim = %d, ldt = %lld", dim, (long long)ldt);
    SAGE_REQUIRE(!grad_rows || max_rows >= 1, "csr_mean_backward_touched: max_rows = %lld with grad_rows", (long long)max_rows);
    SAGE_REQUIRE(self_loop == 0 || self_loop == 1, "csr_mean_backward_touched: self_loop = %d", self_loop);
    SAGE_REQUIRE(rowptr && col && nodes && grad_out && num_rows_out, "csr_mean_backward_touched: NULL array");
    SAGE_REQUIRE(grad_rows || table, "csr_mean_backward_touched: neither grad_rows nor table is given");
    SAGE_REQUIRE(!grad_rows || rows_out, "csr_mean_backward_touched: grad_rows without rows_out");
    TouchedLayout L;
    SAGE_REQUIRE(touched_layout(n, max_edges, num_rows, dim, &L),
                 "csr_mean_backward_touched: n = %d, max_edges = %lld, num_rows = %lld, dim = %d out of range (max_edges + n < 2^31)", n,
                 (long long)max_edges, (long long)num_rows, dim);
    if (const int rc = csr_workspace_check("csr_mean_backward_touched", workspace, workspace_bytes, L.total)) return rc;
    if (n == 0) return SAGE_OK;                          // no term, no launch: num_rows_out and *total_terms are left as they were

    hipStream_t st = (hipStream_t)stream;
    const int R = (int)num_rows, C = (int)L.r.runs_cap;
    SortedTerms T;
    const TermsArgs args{rowptr, col, num_nodes, nodes, n, max_edges, index, num_rows, self_loop, total_terms};
    if (const int rc = rows_sort_terms("csr_mean_backward_touched", args, workspace, L.t, st, &T)) return rc;
    // j'. the run list of the sorted keys: at most C runs, *U.num_runs of them
    RunList U;
    if (const int rc = sorted_run_list(T.keys, (int)T.slots, R, L.r, workspace, num_rows_out, st, &U)) return rc;
    // 1-4. the family's chunk plan and chunk pass with the run list as the row pointer; 5'. the row pass over the runs
    const bool vec4 = (dim % 4 == 0) && (ldg % 4 == 0) && sage_aligned(grad_out, 16) && (!grad_rows || (ldr % 4 == 0 && sage_aligned(grad_rows, 16))) &&
                      (!table || (ldt % 4 == 0 && sage_aligned(table, 16)));
    const BwdSum sum{U.runptr, T.vals, L.r.runs_cap, true, nullptr, C, T.w, nullptr, n, grad_out, ldg, dim, nullptr, 0};
    ChunkPlan P;
    if (const int rc = bwd_chunk_launch(sum, vec4, workspace, L.c, st, &P)) return rc;
    const int blocks = (int)std::min<int64_t>(sage_cdiv(L.r.runs_cap, 4), kNumCU * 8);
#define SAGE_BWD_RUNS(VEC)                                                                                                                  \
    hipLaunchKernelGGL((bwd_runs_row_kernel<VEC>), dim3(blocks), dim3(256), 0, st, U.runptr, T.vals, C, U.num_runs, T.w, grad_out, ldg, dim, \
                       (const int64_t*)P.off, P.cap, (const float*)P.partials, (int64_t)n, U.run_row, rows_out, grad_rows, max_rows, ldr,   \
                       table, ldt, R, lr)
    if (vec4) SAGE_BWD_RUNS(4);
    else SAGE_BWD_RUNS(1);
#undef SAGE_BWD_RUNS
    SAGE_CHECK_LAUNCH("bwd_runs_row_kernel");
    return SAGE_OK;
}
