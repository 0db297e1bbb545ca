// embed_grad: the gradient of a trainable embedding read through the SAMPLED layer-1 sets (aggregators.py:68-71 under the mean of
// aggregators.py:60-74): the forward's nbr1 holds EMBEDDING rows (sage355.engine: col1 = index[col]), so
//     grad_embed[e] = sum over the terms (p, j), t = row_order[p], j < c_t, nbr[t, j] == e, of grad_agg[t] * (1 / c_t)
// sage_gather_mean_backward_ws (sage_backward_det.hip) computes the same sum with one lane group per destination row walking its
// whole run.  With node_degree a few hundred rows share every term of the batch (1.5 M at config-3 size, power-law skewed): a handful
// of lane groups would walk runs of 1e5 terms; and its terms come in ascending frontier ROW order, which is arbitrary (whichever
// lane won the hash slot).  Here the terms are laid out in row_order POSITION, and after the sort the problem is sage_csr_sum with a
// weight per term (sage_csr_sum.hip): long runs are cut into chunks of SAGE_CSR_MEAN_CHUNK terms summed by separate lane groups.
//   1. expand   slot (p, j) -> key = the embedding row (clamped, as det_expand_kernel clamps) or the sentinel embed_rows
//               (padding, dead rows), value = t; 1 / c_t per row
//   2. sort     hipcub::DeviceRadixSort::SortPairs on the key bits that matter: stable, so (p, j) order survives inside a run
//   3. rowptr   rowptr[e] = first position whose key is >= e (a binary search per embedding row): a CSR over the sorted list
//   4-6. count, carry, expand (sage_csr_common.h: csr_chunk_plan): runs of more than one chunk get item entries and partial rows
//   7. chunk    one lane group per item: partials[item] := the chunk's weighted sum
//   8. rows     one lane group per embedding row: short runs summed in place, long ones = their partials in chunk order; STORE
// sage_embed_grad_rows (below) is the same sum for the rows that have a term only, with the SGD update of those rows fused in: steps
// 1, 2, 4-7 unchanged, step 3 a run list of the sorted keys instead of a row pointer over the table, step 8 over the runs.
// Arithmetic of a row (its bits depend on nothing else): p_c = 0, then p_c = fma(g, w, p_c) over chunk c's terms in (p, j) order
// (ONE rounding per term: a fused multiply-add, spelled fmaf so that no compiler flag decides); out = 0 + p_0 + p_1 + ... for a
// run of more than one chunk, out = p_0 for any other.  The terms are weighted_sum's; the item check of step 7 and a row's total are
// sage_csr_common.h's chunk_item and chunked_row_sum (through run_sum), shared with the three CSR files, here with one lane GROUP per
// item or row and therefore without their wave broadcasts.  No float atomics, no host synchronisation, no allocation.
#include "sage_sorted_terms.h"

namespace {

// What both entry points need to lay the terms out and sort them.
struct SortWs {
    SortPairsWs pairs;
    size_t inv_c;
    int slots, bits;
};

bool sort_ws(int32_t n, int32_t k, int64_t embed_rows, int32_t dim, WsCursor& cur, SortWs* S) {
    if (n < 1 || k < 1 || dim < 1 || embed_rows < 1 || embed_rows >= (1ll << 31) || (int64_t)n * k >= (1ll << 31)) return false;
    S->slots = n * k;
    S->bits = sort_key_bits(embed_rows);                           // keys are in [0, embed_rows] (the sentinel included)
    S->pairs.take(S->slots, cur);
    S->inv_c = cur.take((size_t)n * 4);
    return true;
}

struct EmbedLayout {
    SortWs s;
    size_t rowptr, total;
    ChunkWs c;
};

bool embed_layout(int32_t n, int32_t k, int64_t embed_rows, int32_t dim, EmbedLayout* L) {
    WsCursor cur;
    if (!sort_ws(n, k, embed_rows, dim, cur, &L->s)) return false;
    L->rowptr = cur.take((size_t)(embed_rows + 1) * 8);
    if (!chunk_ws(embed_rows, L->s.slots, dim, cur, &L->c)) return false;     // every long run's chunks fit: at most slots terms in all
    L->total = cur.off;
    return true;
}

// 1. one thread per slot, slots in row_order POSITION: slot p * k + j is term j of row t = row_order[p]
__global__ __launch_bounds__(256) void embed_expand_kernel(const int32_t* __restrict__ nbr, const int32_t* __restrict__ cnt, int k, int n,
                                                           const int32_t* __restrict__ n_dev, const int32_t* __restrict__ row_order,
                                                           int embed_rows, int32_t* __restrict__ keys, int32_t* __restrict__ vals,
                                                           float* __restrict__ inv_c) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)n * k) return;
    int nn = n;
    if (n_dev) nn = min(max(*n_dev, 0), n);
    const int p = (int)(i / k), j = (int)(i - (int64_t)p * k);
    const int t = row_order ? row_order[p] : p;
    const bool live = t >= 0 && t < nn;                             // a dead row, or an entry of row_order that names no row
    int key = embed_rows, c = 0;
    if (live) {
        c = min(max(cnt[t], 0), k);
        if (j < c) key = min(max(nbr[(int64_t)t * k + j], 0), embed_rows - 1);      // clamped into the table, as the forward
        if (j == 0) inv_c[t] = c > 0 ? 1.0f / (float)c : 0.f;
    }
    keys[i] = key;
    vals[i] = live ? t : 0;
}

using V4 = float4;

// acc = fma(grad_agg[vals[i]], inv_c[vals[i]], acc) for i in [b, e), in order; 8 rows in flight, and the NEXT 8 row ids requested
// before them, so that a trip of the walk is one memory round trip (ids -> rows would be two: measured 72 us for one 512-term chunk)
__device__ inline void weighted_sum(const float* __restrict__ gagg, int64_t ldg, const int32_t* __restrict__ vals,
                                    const float* __restrict__ inv_c, int64_t b, int64_t e, int c0, V4& acc) {
    if (b >= e) return;
    int r[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) r[u] = vals[min(b + u, e - 1)];
    for (int64_t i = b; i < e; i += 8) {
        int rn[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) rn[u] = vals[min(i + 8 + u, e - 1)];        // stays inside [b, e): the last trip re-reads e - 1
        V4 g[8];
        float w[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            w[u] = inv_c[r[u]];
            g[u] = *reinterpret_cast<const V4*>(gagg + (int64_t)r[u] * ldg + c0);
        }
#pragma unroll
        for (int u = 0; u < 8; ++u)
            if (i + u < e) {
                acc.x = fmaf(g[u].x, w[u], acc.x);
                acc.y = fmaf(g[u].y, w[u], acc.y);
                acc.z = fmaf(g[u].z, w[u], acc.z);
                acc.w = fmaf(g[u].w, w[u], acc.w);
            }
#pragma unroll
        for (int u = 0; u < 8; ++u) r[u] = rn[u];
    }
}

// 7. LG lanes (x 16 B) per item (row, chunk): partials[item] := the chunk's weighted sum
template <int LG>
__global__ __launch_bounds__(256) void embed_chunk_kernel(const float* __restrict__ gagg, int64_t ldg, int dim, const int32_t* __restrict__ vals,
                                                          const float* __restrict__ inv_c, const int64_t* __restrict__ rowptr, int embed_rows,
                                                          const int64_t* __restrict__ off, const int64_t* __restrict__ carry, int nb,
                                                          int64_t cap, const int32_t* __restrict__ item_row, float* __restrict__ partials) {
    const int64_t gid = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / LG, ngroups = ((int64_t)gridDim.x * blockDim.x) / LG;
    const int gl = (int)(threadIdx.x % LG);
    const int64_t items = min(carry[nb], cap);
    const int64_t total = rowptr[embed_rows];
    for (int64_t i = gid; i < items; i += ngroups) {
        int32_t v;
        int64_t cb, ce;
        if (!chunk_item<false>(i, item_row, rowptr, embed_rows, nullptr, embed_rows, total, off, cap, v, cb, ce)) continue;
        for (int c0 = gl * 4; c0 < dim; c0 += LG * 4) {              // dim % 4 == 0 (host-checked)
            V4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
            weighted_sum(gagg, ldg, vals, inv_c, cb, ce, c0, acc);
            *reinterpret_cast<V4*>(partials + i * dim + c0) = acc;
        }
    }
}

// Columns [c0, c0 + 4) of the sum of the run [b, e) of the sorted list, entry r of the row pointer that the chunk pass walked (an
// embedding row for sage_embed_grad, a run for sage_embed_grad_rows): chunked_row_sum over weighted_sum's terms.  With this file's cap
// the chunk pass summed every long run.
__device__ inline V4 run_sum(const float* __restrict__ gagg, int64_t ldg, int dim, const int32_t* __restrict__ vals,
                             const float* __restrict__ inv_c, const int64_t* __restrict__ off, int64_t cap,
                             const float* __restrict__ partials, int64_t r, int64_t b, int64_t e, int c0) {
    const int64_t kc = long_chunks(e - b);
    return chunked_row_sum<V4>(kc, first_item<false>(off, r, kc), cap, partials, dim, c0, true, b, e,
                               [&](int64_t tb, int64_t te, V4& acc) { weighted_sum(gagg, ldg, vals, inv_c, tb, te, c0, acc); });
}

// 8. LG lanes per embedding row
template <int LG>
__global__ __launch_bounds__(256) void embed_row_kernel(const float* __restrict__ gagg, int64_t ldg, int dim, const int32_t* __restrict__ vals,
                                                        const float* __restrict__ inv_c, const int64_t* __restrict__ rowptr, int embed_rows,
                                                        const int64_t* __restrict__ off, int64_t cap, const float* __restrict__ partials,
                                                        float* __restrict__ out, int64_t ld) {
    const int64_t gid = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / LG, ngroups = ((int64_t)gridDim.x * blockDim.x) / LG;
    const int gl = (int)(threadIdx.x % LG);
    const int64_t total = rowptr[embed_rows];
    for (int64_t r = gid; r < embed_rows; r += ngroups) {
        int32_t v;
        int64_t b, e;
        row_span(rowptr, embed_rows, nullptr, (int)r, total, v, b, e);
        for (int c0 = gl * 4; c0 < dim; c0 += LG * 4)
            *reinterpret_cast<V4*>(out + r * ld + c0) = run_sum(gagg, ldg, dim, vals, inv_c, off, cap, partials, r, b, e, c0);
    }
}

// ---- sage_embed_grad_rows: the same sums over the RUNS of the sorted list, nothing sized by embed_rows -----------------------------
// sage_sorted_terms.h's run list of the sorted keys takes the place of the row pointer over the embedding rows; the count / carry /
// expand / chunk kernels above walk it as they walk a CSR of runs_cap = min(slots, embed_rows) rows.
struct RowsLayout {
    SortWs s;
    RunListWs r;
    size_t total;
    ChunkWs c;
};

bool rows_layout(int32_t n, int32_t k, int64_t embed_rows, int32_t dim, RowsLayout* L) {
    WsCursor cur;
    if (!sort_ws(n, k, embed_rows, dim, cur, &L->s)) return false;
    L->r.take(L->s.slots, std::min<int64_t>(L->s.slots, embed_rows), cur);     // distinct rows with a term: what every array below is sized by
    if (!chunk_ws(L->r.runs_cap, L->s.slots, dim, cur, &L->c)) return false;
    L->total = cur.off;
    return true;
}

// 8'. LG lanes per run u < U (U read on the device): the run's sum, run_sum above, stored as row u of the compact gradient (u <
// max_rows) and / or applied to row run_row[u] of the embedding: embed = fma(-lr, sum, embed), one rounding
template <int LG>
__global__ __launch_bounds__(256) void embed_runs_row_kernel(const float* __restrict__ gagg, int64_t ldg, int dim, const int32_t* __restrict__ vals,
                                                             const float* __restrict__ inv_c, const int64_t* __restrict__ runptr, int runs_cap,
                                                             const int64_t* __restrict__ num_runs, const int64_t* __restrict__ off, int64_t cap,
                                                             const float* __restrict__ partials, const int32_t* __restrict__ run_row,
                                                             int32_t* __restrict__ rows_out, float* __restrict__ grad_rows, int64_t max_rows,
                                                             int64_t ldr, float* __restrict__ embed, int64_t lde, int embed_rows, float lr) {
    const int64_t gid = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / LG, ngroups = ((int64_t)gridDim.x * blockDim.x) / LG;
    const int gl = (int)(threadIdx.x % LG);
    const int64_t total = runptr[runs_cap];
    const int64_t nruns = min(*num_runs, (int64_t)runs_cap);
    for (int64_t u = gid; u < nruns; u += ngroups) {
        int32_t v;
        int64_t b, e;
        row_span(runptr, runs_cap, nullptr, (int)u, total, v, b, e);
        const int row = min(max(run_row[u], 0), embed_rows - 1);   // a key of the expand kernel: inside the table already
        const bool keep = grad_rows != nullptr && u < max_rows;
        if (keep && gl == 0) rows_out[u] = row;
        for (int c0 = gl * 4; c0 < dim; c0 += LG * 4) {
            const V4 s = run_sum(gagg, ldg, dim, vals, inv_c, off, cap, partials, u, b, e, c0);
            if (keep) *reinterpret_cast<V4*>(grad_rows + u * ldr + c0) = s;
            if (embed) {
                V4* p = reinterpret_cast<V4*>(embed + (int64_t)row * lde + c0);
                V4 x = *p;
                x.x = fmaf(-lr, s.x, x.x);
                x.y = fmaf(-lr, s.y, x.y);
                x.z = fmaf(-lr, s.z, x.z);
                x.w = fmaf(-lr, s.w, x.w);
                *p = x;
            }
        }
    }
}

// The sorted terms: keys ascending (embedding rows, then the sentinels), vals the set of each term, inv_c the weight of each set
struct SortedTerms {
    const int32_t* keys;
    const int32_t* vals;
    const float* inv_c;
};

// Steps 1-2 of both entry points, errors under the entry's `name`: the sort's temporary is checked before anything is launched.
int sort_terms(const char* name, const int32_t* nbr, const int32_t* cnt, int32_t k, int32_t n, const int32_t* n_dev, const int32_t* row_order,
               int embed_rows, void* workspace, const SortWs& S, hipStream_t st, SortedTerms* T) {
    float* inv_c = (float*)((char*)workspace + S.inv_c);
    if (const int rc = sort_temp_check(name, S.slots, S.bits, S.pairs)) return rc;
    hipLaunchKernelGGL(embed_expand_kernel, dim3(sage_cdiv(S.slots, 256)), dim3(256), 0, st, nbr, cnt, k, n, n_dev, row_order, embed_rows,
                       S.pairs.keys(workspace), S.pairs.vals(workspace), inv_c);
    SAGE_CHECK_LAUNCH("embed_expand_kernel");
    if (const int rc = sort_pairs(name, workspace, S.pairs, S.slots, S.bits, st)) return rc;
    *T = SortedTerms{S.pairs.sorted_keys(workspace), S.pairs.sorted_vals(workspace), inv_c};
    return SAGE_OK;
}

// lanes of 16 bytes per term row: a whole row per trip up to 256 floats
int lane_group(int dim) { return dim >= 256 ? 64 : dim >= 128 ? 32 : dim >= 64 ? 16 : 8; }

#define SAGE_EMBED_LG(KERNEL, BLOCKS, ...)                                                                          \
    do {                                                                                                            \
        if (lg == 64) hipLaunchKernelGGL(KERNEL<64>, dim3(BLOCKS), dim3(256), 0, st, __VA_ARGS__);                   \
        else if (lg == 32) hipLaunchKernelGGL(KERNEL<32>, dim3(BLOCKS), dim3(256), 0, st, __VA_ARGS__);              \
        else if (lg == 16) hipLaunchKernelGGL(KERNEL<16>, dim3(BLOCKS), dim3(256), 0, st, __VA_ARGS__);              \
        else hipLaunchKernelGGL(KERNEL<8>, dim3(BLOCKS), dim3(256), 0, st, __VA_ARGS__);                             \
    } while (0)

// The chunk split of the `rows` rows of `rowptr` over the sorted list (the embedding rows, or the runs), and the chunk pass
int chunk_pass(const float* grad_agg, int64_t ldg, int32_t dim, const SortedTerms& T, const int64_t* rowptr, int rows, void* workspace,
               const ChunkWs& C, hipStream_t st, ChunkPlan* P) {
    if (const int rc = csr_chunk_plan(rowptr, rows, nullptr, rows, workspace, C, st, P)) return rc;
    if (P->cap > 0) {
        const int lg = lane_group(dim);
        const int blocks = (int)std::min<int64_t>((P->cap * lg + 255) / 256, kNumCU * 8);
        SAGE_EMBED_LG(embed_chunk_kernel, blocks, grad_agg, ldg, dim, T.vals, T.inv_c, rowptr, rows, (const int64_t*)P->off,
                      (const int64_t*)P->carry, P->nb, P->cap, (const int32_t*)P->item_row, P->partials);
        SAGE_CHECK_LAUNCH("embed_chunk_kernel");
    }
    return SAGE_OK;
}

}  // namespace

extern "C" size_t sage_embed_grad_workspace_bytes(int32_t n, int32_t k, int64_t embed_rows, int32_t dim) {
    if (n == 0 && k >= 1 && dim >= 1 && embed_rows >= 1) return 256;
    EmbedLayout L;
    return embed_layout(n, k, embed_rows, dim, &L) ? L.total : 0;
}

extern "C" int sage_embed_grad(const float* grad_agg, int64_t ldg, int32_t dim, const int32_t* nbr, const int32_t* cnt, int32_t k, int32_t n,
                               const int32_t* n_dev, const int32_t* row_order, float* grad_embed, int64_t embed_rows, int64_t ld,
                               void* workspace, size_t workspace_bytes, sage_stream_t stream) {
    // shapes first, then pointers: a bad shape is reported as such whatever the pointers are
    SAGE_REQUIRE(n >= 0 && k >= 1 && (int64_t)n * k < (1ll << 31), "embed_grad: n = %d, k = %d (n * k < 2^31)", n, k);
    SAGE_REQUIRE(dim >= 4 && dim % 4 == 0, "embed_grad: dim = %d (rows of 16-byte pieces)", dim);
    SAGE_REQUIRE(ldg >= dim && ldg % 4 == 0, "embed_grad: ldg = %lld", (long long)ldg);
    SAGE_REQUIRE(ld >= dim && ld % 4 == 0, "embed_grad: ld = %lld", (long long)ld);
    SAGE_REQUIRE(embed_rows >= 1 && embed_rows < (1ll << 31), "embed_grad: embed_rows = %lld", (long long)embed_rows);
    SAGE_REQUIRE(grad_agg && nbr && cnt && grad_embed, "embed_grad: NULL array");
    SAGE_REQUIRE(sage_aligned(grad_agg, 16) && sage_aligned(grad_embed, 16), "embed_grad: grad_agg / grad_embed not 16-byte aligned");
    if (n == 0) return SAGE_OK;
    EmbedLayout L;
    SAGE_REQUIRE(embed_layout(n, k, embed_rows, dim, &L), "embed_grad: n = %d, k = %d, embed_rows = %lld, dim = %d out of range", n, k,
                 (long long)embed_rows, dim);
    if (const int rc = csr_workspace_check("embed_grad", workspace, workspace_bytes, L.total)) return rc;
    hipStream_t st = (hipStream_t)stream;
    int64_t* rowptr = (int64_t*)((char*)workspace + L.rowptr);
    const int R = (int)embed_rows;
    SortedTerms T;
    if (const int rc = sort_terms("embed_grad", nbr, cnt, k, n, n_dev, row_order, R, workspace, L.s, st, &T)) return rc;
    hipLaunchKernelGGL(sorted_rowptr_kernel, dim3(sage_cdiv(embed_rows + 1, 256)), dim3(256), 0, st, T.keys, L.s.slots, R, rowptr);
    SAGE_CHECK_LAUNCH("sorted_rowptr_kernel");
    ChunkPlan P;
    if (const int rc = chunk_pass(grad_agg, ldg, dim, T, rowptr, R, workspace, L.c, st, &P)) return rc;
    const int lg = lane_group(dim);
    const int blocks = (int)std::min<int64_t>((embed_rows * lg + 255) / 256, kNumCU * 8);
    SAGE_EMBED_LG(embed_row_kernel, blocks, grad_agg, ldg, dim, T.vals, T.inv_c, (const int64_t*)rowptr, R, (const int64_t*)P.off, P.cap,
                  (const float*)P.partials, grad_embed, ld);
    SAGE_CHECK_LAUNCH("embed_row_kernel");
    return SAGE_OK;
}

extern "C" size_t sage_embed_grad_rows_workspace_bytes(int32_t n, int32_t k, int64_t embed_rows, int32_t dim) {
    if (n == 0 && k >= 1 && dim >= 1 && embed_rows >= 1) return 256;
    RowsLayout L;
    return rows_layout(n, k, embed_rows, dim, &L) ? L.total : 0;
}

extern "C" int sage_embed_grad_rows(const float* grad_agg, int64_t ldg, int32_t dim, const int32_t* nbr, const int32_t* cnt, int32_t k, int32_t n,
                                    const int32_t* n_dev, const int32_t* row_order, int64_t embed_rows, int32_t* num_rows_out,
                                    int32_t* rows_out, float* grad_rows, int64_t max_rows, int64_t ldr, float* embed, int64_t lde, float lr,
                                    void* workspace, size_t workspace_bytes, sage_stream_t stream) {
    // sage_embed_grad's rules and order: shapes first, then pointers
    SAGE_REQUIRE(n >= 0 && k >= 1 && (int64_t)n * k < (1ll << 31), "embed_grad_rows: n = %d, k = %d (n * k < 2^31)", n, k);
    SAGE_REQUIRE(dim >= 4 && dim % 4 == 0, "embed_grad_rows: dim = %d (rows of 16-byte pieces)", dim);
    SAGE_REQUIRE(ldg >= dim && ldg % 4 == 0, "embed_grad_rows: ldg = %lld", (long long)ldg);
    SAGE_REQUIRE(!grad_rows || (ldr >= dim && ldr % 4 == 0), "embed_grad_rows: ldr = %lld", (long long)ldr);
    SAGE_REQUIRE(!embed || (lde >= dim && lde % 4 == 0), "embed_grad_rows: lde = %lld", (long long)lde);
    SAGE_REQUIRE(embed_rows >= 1 && embed_rows < (1ll << 31), "embed_grad_rows: embed_rows = %lld", (long long)embed_rows);
    SAGE_REQUIRE(!grad_rows || max_rows >= 1, "embed_grad_rows: max_rows = %lld with grad_rows", (long long)max_rows);
    SAGE_REQUIRE(grad_agg && nbr && cnt && num_rows_out, "embed_grad_rows: NULL array");
    SAGE_REQUIRE(grad_rows || embed, "embed_grad_rows: neither grad_rows nor embed is given");
    SAGE_REQUIRE(!grad_rows || rows_out, "embed_grad_rows: grad_rows without rows_out");
    SAGE_REQUIRE(sage_aligned(grad_agg, 16) && sage_aligned(grad_rows, 16) && sage_aligned(embed, 16),
                 "embed_grad_rows: grad_agg / grad_rows / embed not 16-byte aligned");
    if (n == 0) return SAGE_OK;
    RowsLayout L;
    SAGE_REQUIRE(rows_layout(n, k, embed_rows, dim, &L), "embed_grad_rows: n = %d, k = %d, embed_rows = %lld, dim = %d out of range", n, k,
                 (long long)embed_rows, dim);
    if (const int rc = csr_workspace_check("embed_grad_rows", workspace, workspace_bytes, L.total)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const int R = (int)embed_rows, C = (int)L.r.runs_cap;
    SortedTerms T;
    if (const int rc = sort_terms("embed_grad_rows", nbr, cnt, k, n, n_dev, row_order, R, workspace, L.s, st, &T)) return rc;
    // the run list (sage_sorted_terms.h): count the heads per tile, scan the tiles, write the runs, close the list
    RunList U;
    if (const int rc = sorted_run_list(T.keys, L.s.slots, R, L.r, workspace, num_rows_out, st, &U)) return rc;
    // the chunk split over the runs: sage_embed_grad's launches with the run list as the row pointer
    ChunkPlan P;
    if (const int rc = chunk_pass(grad_agg, ldg, dim, T, U.runptr, C, workspace, L.c, st, &P)) return rc;
    const int lg = lane_group(dim);
    const int blocks = (int)std::min<int64_t>((L.r.runs_cap * lg + 255) / 256, kNumCU * 8);
    SAGE_EMBED_LG(embed_runs_row_kernel, blocks, grad_agg, ldg, dim, T.vals, T.inv_c, U.runptr, C, U.num_runs, (const int64_t*)P.off, P.cap,
                  (const float*)P.partials, U.run_row, rows_out, grad_rows, max_rows, ldr, embed, lde, R, lr);
#undef SAGE_EMBED_LG
    SAGE_CHECK_LAUNCH("embed_runs_row_kernel");
    return SAGE_OK;
}
