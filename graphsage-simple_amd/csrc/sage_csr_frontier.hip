// csr_frontier: the frontier of a FULL-neighbourhood hop (aggregators.py:47-48 num_sample=None, then 52-53): the distinct ids among a
// seed batch and every neighbour of every seed, with an id -> row map.  The hash frontier (sage_sample.hip) takes padded [n, k] lists
// with k <= 64; a whole row can hold 62,333 ids (configs[2]'s hub), so this one walks the CSR itself and keeps the map as a plain
// int32 [num_nodes] array `pos` (-1 = not in the set) -- which is exactly the `index` sage_csr_mean_indexed reads rows through.
//
// Load balance is csr_mean's, from sage_csr_common.h (csr_chunk_plan / chunk_item / row_span; no second copy of the split): a seed row
// longer than SAGE_CSR_MEAN_CHUNK entries is cut into chunks, each walked by a wave of its own; a long row whose items do not fit the
// workspace (max_edges below the truth) is walked whole by its row wave -- slower, same set.
//
// Launches, all on the caller's stream, no host round trip: count, carry, expand (the plan), then ONE claim kernel with three loops
//   seeds   64 seeds per wave trip, a lane each: the seed itself joins the set
//   rows    a wave per seed: the row's entries, unless the chunk pass has them
//   items   a wave per chunk of a long row
// Claiming an id u (claim() below): a relaxed load skips ids somebody already holds (pos only ever moves away from -1 during the
// kernel, so a stale -1 merely falls through to the CAS); atomicCAS(&pos[u], -1, kClaimed) picks ONE winner per id; the winners of a
// wave reserve their rows with one atomicAdd on *count (ballot + popcount, as sage_sample_wide.hip does: thousands of waves share that
// one counter -- cdna_hip_programming.md Guideline 12) and store row -> pos[u], u -> nodes_out[row].  Losers do nothing and nobody
// reads a ROW out of pos here, so no wave ever waits for another.  Integer atomics only; the order of nodes_out is arbitrary, its
// content as a set and pos as its inverse are not.
#include "sage_csr_common.h"

namespace {

constexpr int32_t kClaimed = -2;   // pos[u] between the winner's CAS and its store of the row; never left behind

struct FrontierLayout {
    ChunkWs c;
    size_t total;
};

bool frontier_layout(int32_t n, int64_t max_edges, FrontierLayout* L) {
    if (n < 0 || max_edges < 0) return false;
    WsCursor cur;
    if (!chunk_ws(n, max_edges, 0, cur, &L->c)) return false;     // dim 0: the split's lists without partial sums
    L->total = cur.off;
    return true;
}

struct FrontierOut {
    int32_t* pos;         // [num_nodes]
    int32_t* nodes_out;   // [max_nodes]
    int32_t* count;       // [1]
    int num_nodes;
    int max_nodes;
};

// Every lane of the wave calls this (ballot); u < 0 or >= num_nodes: the lane claims nothing.
__device__ inline void claim(int32_t u, const FrontierOut& f, int lane) {
    bool won = false;
    if (u >= 0 && u < f.num_nodes && __hip_atomic_load(&f.pos[u], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == -1)
        won = atomicCAS(&f.pos[u], -1, kClaimed) == -1;
    const unsigned long long wb = __ballot(won);
    if (wb == 0ull) return;
    int base = 0;
    if (lane == 0) base = atomicAdd(f.count, __popcll(wb));
    base = __builtin_amdgcn_readfirstlane(base);
    if (won) {
        const int row = base + __popcll(wb & ((1ull << lane) - 1ull));
        f.pos[u] = row;
        if ((uint32_t)row < (uint32_t)f.max_nodes) f.nodes_out[row] = u;     // past the end: counted, not stored
    }
}

// col[b..e), b and e wave-uniform and inside col[] (row_span / chunk_item clamp them)
__device__ inline void claim_edges(const int32_t* __restrict__ col, int64_t b, int64_t e, const FrontierOut& f, int lane) {
    for (int64_t base = b; base < e; base += kWave) claim(base + lane < e ? col[base + lane] : -1, f, lane);
}

__global__ __launch_bounds__(256) void csr_frontier_kernel(const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col, int64_t num_nodes,
                                                           const int32_t* __restrict__ seeds, int n, const int64_t* __restrict__ off,
                                                           const int64_t* __restrict__ carry, int nb, int64_t cap,
                                                           const int32_t* __restrict__ item_row, FrontierOut f) {
    const int lane = sage_lane();
    const int64_t wave = (int64_t)((blockIdx.x * blockDim.x + threadIdx.x) >> 6);
    const int64_t nwaves = (int64_t)((gridDim.x * blockDim.x) >> 6);
    const int64_t total = rowptr[num_nodes];
    for (int64_t s0 = wave * kWave; s0 < n; s0 += nwaves * kWave) claim(s0 + lane < n ? seeds[s0 + lane] : -1, f, lane);
    for (int64_t r = wave; r < n; r += nwaves) {
        int32_t v;
        int64_t b, e;
        row_span<true>(rowptr, num_nodes, seeds, (int)r, total, v, b, e);
        const int64_t k = long_chunks(e - b);
        if (chunks_fit(k, first_item<true>(off, r, k), cap)) continue;       // the items loop walks this row
        claim_edges(col, b, e, f, lane);
    }
    const int64_t items = min(carry[nb], cap);
    for (int64_t i = wave; i < items; i += nwaves) {
        int32_t v;
        int64_t cb, ce;
        if (chunk_item<true>(i, item_row, rowptr, num_nodes, seeds, n, total, off, cap, v, cb, ce)) claim_edges(col, cb, ce, f, lane);
    }
}

__global__ __launch_bounds__(256) void csr_frontier_clear_kernel(int32_t* __restrict__ pos, const int32_t* __restrict__ nodes_out,
                                                                 const int32_t* __restrict__ count, int max_nodes) {
    const int rows = min(max(*count, 0), max_nodes);
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < rows; i += gridDim.x * blockDim.x) {
        const int32_t u = nodes_out[i];
        if (u >= 0) pos[u] = -1;
    }
}

}  // namespace

extern "C" size_t sage_csr_frontier_workspace_bytes(int32_t n, int64_t max_edges) {
    FrontierLayout L;
    return frontier_layout(n, max_edges, &L) ? L.total : 0;
}

extern "C" int sage_csr_frontier(const int64_t* rowptr, const int32_t* col, int64_t num_nodes, const int32_t* seeds, int32_t n,
                                 int64_t max_edges, int32_t* pos, int32_t* nodes_out, int32_t max_nodes, int32_t* count, void* workspace,
                                 size_t workspace_bytes, sage_stream_t stream) {
    SAGE_REQUIRE(num_nodes >= 0 && num_nodes < (1ll << 31), "csr_frontier: num_nodes = %lld", (long long)num_nodes);
    SAGE_REQUIRE(n >= 0, "csr_frontier: n = %d", n);
    SAGE_REQUIRE(max_nodes >= 0, "csr_frontier: max_nodes = %d", max_nodes);
    SAGE_REQUIRE(max_edges >= 0, "csr_frontier: max_edges = %lld", (long long)max_edges);
    SAGE_REQUIRE(rowptr && col && seeds && pos && nodes_out && count, "csr_frontier: NULL array");
    FrontierLayout L;
    SAGE_REQUIRE(frontier_layout(n, max_edges, &L), "csr_frontier: n = %d, max_edges = %lld out of range", n, (long long)max_edges);
    if (const int rc = csr_workspace_check("csr_frontier", workspace, workspace_bytes, L.total)) return rc;
    if (n == 0) return SAGE_OK;

    hipStream_t st = (hipStream_t)stream;
    ChunkPlan P;
    if (const int rc = csr_chunk_plan(rowptr, num_nodes, seeds, n, workspace, L.c, st, &P)) return rc;
    const int blocks = (int)std::min<int64_t>(((int64_t)n + P.cap + 3) / 4, kNumCU * 8);
    hipLaunchKernelGGL(csr_frontier_kernel, dim3(blocks), dim3(256), 0, st, rowptr, col, num_nodes, seeds, n, (const int64_t*)P.off,
                       (const int64_t*)P.carry, P.nb, P.cap, (const int32_t*)P.item_row, FrontierOut{pos, nodes_out, count, (int)num_nodes, max_nodes});
    SAGE_CHECK_LAUNCH("csr_frontier_kernel");
    return SAGE_OK;
}

extern "C" int sage_csr_frontier_clear(int32_t* pos, const int32_t* nodes_out, const int32_t* count, int32_t max_nodes, sage_stream_t stream) {
    SAGE_REQUIRE(max_nodes >= 0, "csr_frontier_clear: max_nodes = %d", max_nodes);
    SAGE_REQUIRE(pos && nodes_out && count, "csr_frontier_clear: NULL array");
    if (max_nodes == 0) return SAGE_OK;
    hipLaunchKernelGGL(csr_frontier_clear_kernel, dim3(std::min(sage_cdiv(max_nodes, 256), kNumCU * 8)), dim3(256), 0, (hipStream_t)stream, pos,
                       nodes_out, count, max_nodes);
    SAGE_CHECK_LAUNCH("csr_frontier_clear_kernel");
    return SAGE_OK;
}
