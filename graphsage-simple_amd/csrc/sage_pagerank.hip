// pagerank: the power iteration behind the reference's `pagerank` initializer (model.py:158-162, 322-326, 470-474: nx.pagerank(G)
// as the single feature column), one step per call, as a PULL over a CSR whose row i lists the nodes that link to i:
//     s_i      = sum over row i's entries e of y[col[e]]             y = x * inv_out, 4 bytes gathered per entry
//     x_next_i = alpha * (s_i + mass / N) + (1 - alpha) / N          mass = sum of x_j over the dangling nodes (inv_out[j] == 0)
//     y_next_i = x_next_i * inv_out[i]                               stored beside x_next: the next step gathers it directly
//     err      = sum over i of |x_next_i - x_i|                      next mass = sum of x_next_j over the dangling nodes
// nx.pagerank's iteration with its defaults (uniform start, personalization and dangling weights); the caller compares err with
// N * tol (ops.pagerank).
//
// LANES WORK ON ENTRIES.  A table row here is ONE float, so sage_csr_common.h's sum_edges (a wave per row, a lane per column
// group) would keep one lane of 64 busy.  Instead a row belongs to a GROUP of kPrGroup lanes and a wave holds 64 / kPrGroup rows;
// the group's lanes take the row's entries side by side.
//
// ORDER OF A ROW'S SUM (the bits of x_next[i] depend on row i's stored entries, y and the step's three scalars alone -- not on N's
// cut into blocks, on the rows beside it, on the grid, on kPrGroup, on kPrRows or on how many trips are loaded together):
//   span   A span is at most SAGE_CSR_MEAN_CHUNK consecutive entries [b, e).  It has 64 SLOTS; slot j = 0 + t_j + t_(j+64) +
//          t_(j+128) + ... in that order, t_p = y[clamp(col[b + p])] (an absent entry adds nothing).  The slots are folded in
//          halves: slot j += slot j + 32, then + 16, + 8, + 4, + 2, + 1; slot 0 is the span's sum.  A lane owns the slots
//          gl, gl + kPrGroup, ...: the first folds are adds between its own registers, the rest are shuffles inside the group.  A slot
//          sum is never -0 (it starts from +0) and s + (+0) = s, so the empty slots of a short row change nothing and every group
//          width folds the same bits.
//   row    A row of at most SAGE_CSR_MEAN_CHUNK entries is one span: s_i = 0 + span.  A longer row is cut into chunks of that many
//          by the shared planner (sage_csr_common.h: csr_chunk_plan), every chunk is a span summed by its own group into
//          partials[item] = 0 + span, and s_i = 0 + p_0 + p_1 + ... in chunk order (chunked_row_sum, which also redoes the chunks
//          in place, same operations, for a long row that found no workspace room).
//   x_next dm = mass / float(N), tele = (1 - alpha) / float(N), x_next_i = fma(alpha, s_i + dm, tele), y_next_i = x_next_i * inv_out[i].
// ORDER OF err AND mass (no float atomics; they stay on the device as two floats): a block owns a TILE of kPrTile consecutive
// rows and writes their terms |x_next_i - x_i| and (inv_out[i] == 0 ? x_next_i : 0) into LDS (0 for a row past N).  Thread t adds
// terms t, t + 256, ... of the tile in that order, a wave folds its 64 values in halves (+32 ... +1), thread 0 adds the four wave
// sums in wave order and stores the tile's pair.  One further block (the fixed-order reduce of sage_head.hip, here over tiles):
// thread t adds the pairs of tiles t, t + 256, ... in that order, then the same fold; thread 0 stores state = {err, mass} with
// plain stores.  So err and mass depend on N and the values, never on the grid or on timing.
//
// Launches.  sage_pagerank_init / sage_pagerank_load: the planner's count, carry, expand over all N rows (the plan depends on rowptr
// alone, so it is made ONCE and every step reads it from the workspace), prepare (x, inv_out, y, the mass terms), reduce.
// sage_pagerank_step: chunk (only if the workspace has room for items), step, reduce.  col is streamed once per step; y is the
// only gathered array (4 MiB at 2^20 nodes: one XCD's L2; 32 MiB at 2^23: inside the Infinity Cache).
// A workspace that no init filled for this rowptr gives wrong numbers, never an access out of range: chunk_item refuses an item
// that names no row, a negative first item counts as "no room", and every id from col is clamped into [0, N).
#include "sage_csr_common.h"

namespace {

#ifndef SAGE_PAGERANK_GROUP
#define SAGE_PAGERANK_GROUP 16
#endif
constexpr int kPrGroup = SAGE_PAGERANK_GROUP;          // lanes of a row; changes the speed, never a bit
constexpr int kPrPerLane = kWave / kPrGroup;           // slots of a lane
constexpr int kPrThreads = 256;
constexpr int kPrWaves = kPrThreads / kWave;
constexpr int kPrGroups = kPrThreads / kPrGroup;       // rows a block walks side by side
constexpr int kPrTile = 512;                           // rows of a block = one (err, mass) partial: fixes the order of err and mass
#ifndef SAGE_PAGERANK_ROWS
#define SAGE_PAGERANK_ROWS 2
#endif
constexpr int kPrRows = SAGE_PAGERANK_ROWS;            // rows of a group in flight together; changes the speed, never a bit
static_assert(kPrGroup == 8 || kPrGroup == 16 || kPrGroup == 32 || kPrGroup == 64, "a group is a power-of-two part of a wave");
static_assert(kPrTile % kPrThreads == 0 && kPrTile % (kPrGroups * kPrRows) == 0, "a tile is whole trips of the block");
static_assert(kChunk % kWave == 0, "a span is whole trips of 64 slots");

struct PrLayout {
    ChunkWs c;
    size_t tile_part;   // float [tiles][2]: err, mass
    int64_t tiles;
    size_t total;
};

bool pr_layout(int64_t num_nodes, int64_t num_edges, PrLayout* L) {
    if (num_nodes < 1 || num_nodes >= (1ll << 31) || num_edges < 0) return false;
    WsCursor cur;
    if (!chunk_ws(num_nodes, num_edges, 1, cur, &L->c)) return false;
    L->tiles = (num_nodes + kPrTile - 1) / kPrTile;
    L->tile_part = cur.take((size_t)L->tiles * 2 * sizeof(float));
    L->total = cur.off;
    return true;
}

// The slots of span [b, e) (see ORDER above) from entry b0 on, added to a[]: b0 - b is a multiple of 64 and a[] holds the slots of
// the entries before b0.  b0, e are the same in the group's lanes; gl = the lane's place in its group.  Ids are clamped into
// [0, last].  Two trips (128 entries) are loaded together; a slot still adds its entries in stored order.
__device__ inline void span_rest(const int32_t* __restrict__ col, const float* __restrict__ y, int last, int64_t b0, int64_t e, int gl,
                                 float (&a)[kPrPerLane]) {
    constexpr int kTrips = 2;
    for (int64_t base = b0 + gl; base - gl < e; base += kTrips * kWave) {          // the group leaves the loop together
        int id[kTrips][kPrPerLane];
        float t[kTrips][kPrPerLane];
#pragma unroll
        for (int j = 0; j < kTrips; ++j)
#pragma unroll
            for (int u = 0; u < kPrPerLane; ++u) {
                const int64_t p = base + j * kWave + u * kPrGroup;
                id[j][u] = p < e ? col[p] : 0;
            }
#pragma unroll
        for (int j = 0; j < kTrips; ++j)
#pragma unroll
            for (int u = 0; u < kPrPerLane; ++u) {
                const int64_t p = base + j * kWave + u * kPrGroup;
                t[j][u] = p < e ? y[min(max(id[j][u], 0), last)] : 0.f;
            }
#pragma unroll
        for (int j = 0; j < kTrips; ++j)
#pragma unroll
            for (int u = 0; u < kPrPerLane; ++u) a[u] += t[j][u];
    }
}

// The slots folded in halves: the same value in every lane of the group.
__device__ inline float span_fold(float (&a)[kPrPerLane]) {
#pragma unroll
    for (int s = kPrPerLane / 2; s >= 1; s >>= 1)                       // slot strides 32 ... kPrGroup: the lane's own registers
#pragma unroll
        for (int u = 0; u < s; ++u) a[u] += a[u + s];
    float v = a[0];
#pragma unroll
    for (int s = kPrGroup / 2; s >= 1; s >>= 1) v += __shfl_xor(v, s, kPrGroup);   // x + y = y + x: every lane folds slot 0's bits
    return v;
}

// The sum of span [b, e)
__device__ inline float span_sum(const int32_t* __restrict__ col, const float* __restrict__ y, int last, int64_t b, int64_t e, int gl) {
    float a[kPrPerLane];
#pragma unroll
    for (int u = 0; u < kPrPerLane; ++u) a[u] = 0.f;
    span_rest(col, y, last, b, e, gl, a);
    return span_fold(a);
}

// The block's sums of one value pair per thread: a wave folds in halves, thread 0 adds the wave sums in wave order.  Result in
// thread 0.  Every thread of the block calls this, once per kernel.
__device__ inline void block_sum2(float& a, float& b) {
    __shared__ float wa[kPrWaves], wb[kPrWaves];
#pragma unroll
    for (int s = kWave / 2; s >= 1; s >>= 1) {
        a += __shfl_xor(a, s, kWave);
        b += __shfl_xor(b, s, kWave);
    }
    if (sage_lane() == 0) {
        wa[threadIdx.x / kWave] = a;
        wb[threadIdx.x / kWave] = b;
    }
    __syncthreads();
    a = wa[0];
    b = wb[0];
#pragma unroll
    for (int w = 1; w < kPrWaves; ++w) {
        a += wa[w];
        b += wb[w];
    }
}

// One group per item (row, chunk): partials[item] := 0 + the chunk's span
__global__ __launch_bounds__(kPrThreads) void pagerank_chunk_kernel(const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                                     int64_t num_nodes, const float* __restrict__ y,
                                                                     const int64_t* __restrict__ off, const int64_t* __restrict__ carry, int nb,
                                                                     int64_t cap, const int32_t* __restrict__ item_row,
                                                                     float* __restrict__ partials) {
    const int gl = threadIdx.x % kPrGroup;
    const int64_t group = ((int64_t)blockIdx.x * kPrThreads + threadIdx.x) / kPrGroup;
    const int64_t ngroups = (int64_t)gridDim.x * kPrGroups;
    const int n = (int)num_nodes;
    const int64_t items = min(carry[nb], cap);
    const int64_t total = rowptr[num_nodes];
    for (int64_t i = group; i < items; i += ngroups) {
        int32_t v;
        int64_t cb, ce;
        if (!chunk_item<false>(i, item_row, rowptr, num_nodes, nullptr, n, total, off, cap, v, cb, ce)) continue;
        float acc = 0.f;
        acc += span_sum(col, y, n - 1, cb, ce, gl);
        if (gl == 0) partials[i] = acc;
    }
}

// One block per tile of kPrTile rows, one group per row, kPrRows rows of a group in flight together: the tile's row pointers are
// staged in LDS (one coalesced read instead of a dependent load in front of every row), then a trip issues the first 64 ids of its
// kPrRows rows, then their y values, and only then adds -- two memory latencies per kPrRows rows instead of three per row.  A row of
// more than 64 entries goes on in span_rest; a row of more than one chunk has nothing preloaded (its partials are its sum).
__global__ __launch_bounds__(kPrThreads) void pagerank_step_kernel(const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                                    int64_t num_nodes, const float* __restrict__ inv_out, float alpha,
                                                                    const float* __restrict__ x, const float* __restrict__ y,
                                                                    float* __restrict__ x_next, float* __restrict__ y_next,
                                                                    const float* __restrict__ state, const int64_t* __restrict__ off,
                                                                    int64_t cap, const float* __restrict__ partials,
                                                                    float* __restrict__ tile_part) {
    __shared__ int64_t rp_sh[kPrTile + 1];
    __shared__ float err_sh[kPrTile], mass_sh[kPrTile];
    const int n = (int)num_nodes;
    const int gl = threadIdx.x % kPrGroup, gi = threadIdx.x / kPrGroup;
    const int64_t total = rowptr[num_nodes];
    const float nf = (float)n;
    const float dm = state[1] / nf;
    const float tele = (1.f - alpha) / nf;
    const int64_t tile0 = (int64_t)blockIdx.x * kPrTile;
    const int rows = (int)min((int64_t)kPrTile, num_nodes - tile0);
    // row_span's rule on the staged pointers: each clamped into [0, total] here, e = max(e, b) where a row is read
    for (int i = threadIdx.x; i <= rows; i += kPrThreads) rp_sh[i] = min(max(rowptr[tile0 + i], (int64_t)0), total);
    __syncthreads();
    for (int t0 = gi; t0 < kPrTile; t0 += kPrGroups * kPrRows) {
        int64_t b[kPrRows], e[kPrRows], k[kPrRows];
        int id[kPrRows][kPrPerLane];
        float pre[kPrRows][kPrPerLane], xi[kPrRows], io[kPrRows];
#pragma unroll
        for (int q = 0; q < kPrRows; ++q) {
            const int t = t0 + q * kPrGroups;
            const bool live = t < rows;                                 // the same in the group's lanes
            b[q] = live ? rp_sh[t] : 0;
            e[q] = live ? max(rp_sh[t + 1], b[q]) : 0;
            k[q] = long_chunks(e[q] - b[q]);
            const int64_t fe = k[q] == 0 ? e[q] : b[q];
#pragma unroll
            for (int u = 0; u < kPrPerLane; ++u) {
                const int64_t p = b[q] + u * kPrGroup + gl;
                id[q][u] = p < fe ? col[p] : 0;
            }
            xi[q] = live ? x[tile0 + t] : 0.f;
            io[q] = live ? inv_out[tile0 + t] : 0.f;
        }
#pragma unroll
        for (int q = 0; q < kPrRows; ++q) {
            const int64_t fe = k[q] == 0 ? e[q] : b[q];
#pragma unroll
            for (int u = 0; u < kPrPerLane; ++u) pre[q][u] = b[q] + u * kPrGroup + gl < fe ? y[min(max(id[q][u], 0), n - 1)] : 0.f;
        }
#pragma unroll
        for (int q = 0; q < kPrRows; ++q) {
            const int t = t0 + q * kPrGroups;
            float d = 0.f, m = 0.f;
            if (t < rows) {
                const int r = (int)(tile0 + t);
                int64_t o = first_item<false>(off, r, k[q]);
                if (o < 0) o = cap;                                     // no plan in this workspace: sum in place
                const float s = chunked_row_sum<float>(k[q], o, cap, partials, 1, 0, true, b[q], e[q], [&](int64_t tb, int64_t te, float& acc) {
                    float a[kPrPerLane];
                    const bool first = k[q] == 0;                       // the whole row as one span: its first trip is in pre[q]
#pragma unroll
                    for (int u = 0; u < kPrPerLane; ++u) a[u] = first ? 0.f + pre[q][u] : 0.f;
                    span_rest(col, y, n - 1, first ? tb + kWave : tb, te, gl, a);
                    acc += span_fold(a);
                });
                const float xn = __builtin_fmaf(alpha, s + dm, tele);
                if (gl == 0) {
                    x_next[r] = xn;
                    y_next[r] = xn * io[q];
                }
                d = fabsf(xn - xi[q]);
                m = io[q] == 0.f ? xn : 0.f;
            }
            if (gl == 0) {
                err_sh[t] = d;
                mass_sh[t] = m;
            }
        }
    }
    __syncthreads();
    float a = err_sh[threadIdx.x], c = mass_sh[threadIdx.x];
#pragma unroll
    for (int q = 1; q < kPrTile / kPrThreads; ++q) {
        a += err_sh[q * kPrThreads + threadIdx.x];
        c += mass_sh[q * kPrThreads + threadIdx.x];
    }
    block_sum2(a, c);
    if (threadIdx.x == 0) {
        tile_part[2 * (int64_t)blockIdx.x] = a;
        tile_part[2 * (int64_t)blockIdx.x + 1] = c;
    }
}

// The start of an iteration, one block per tile, a thread per row.  INIT: x = 1 / N, inv_out = 1 / out-degree (0: dangling) are
// written; else both are the caller's.  y = x * inv_out, the tile's pair = (0, its dangling mass).
template <bool INIT>
__global__ __launch_bounds__(kPrThreads) void pagerank_prepare_kernel(const int64_t* __restrict__ rowptr, int64_t num_nodes,
                                                                       const int32_t* __restrict__ out_degree, float* __restrict__ x,
                                                                       float* __restrict__ y, float* __restrict__ inv_out,
                                                                       float* __restrict__ tile_part) {
    const int n = (int)num_nodes;
    const int64_t total = rowptr[num_nodes];
    const float x0 = 1.f / (float)n;
    const int64_t tile0 = (int64_t)blockIdx.x * kPrTile;
    float zero = 0.f, m = 0.f;
#pragma unroll
    for (int q = 0; q < kPrTile / kPrThreads; ++q) {
        const int64_t r64 = tile0 + q * kPrThreads + threadIdx.x;
        if (r64 >= n) continue;
        const int r = (int)r64;
        float xi, io;
        if constexpr (INIT) {
            int64_t deg;
            if (out_degree) {
                deg = out_degree[r];
            } else {
                int32_t v;
                int64_t b, e;
                row_span(rowptr, num_nodes, nullptr, r, total, v, b, e);
                deg = e - b;
            }
            xi = x0;
            io = deg > 0 ? 1.f / (float)deg : 0.f;
            x[r] = xi;
            inv_out[r] = io;
        } else {
            xi = x[r];
            io = inv_out[r];
        }
        y[r] = xi * io;
        m += io == 0.f ? xi : 0.f;
    }
    block_sum2(zero, m);
    if (threadIdx.x == 0) {
        tile_part[2 * (int64_t)blockIdx.x] = 0.f;
        tile_part[2 * (int64_t)blockIdx.x + 1] = m;
    }
}

// One block: state = {err, mass} = the tiles' pairs added in the fixed order of the header.
__global__ __launch_bounds__(kPrThreads) void pagerank_reduce_kernel(const float* __restrict__ tile_part, int64_t tiles,
                                                                      float* __restrict__ state) {
    float a = 0.f, c = 0.f;
    for (int64_t j = threadIdx.x; j < tiles; j += kPrThreads) {
        a += tile_part[2 * j];
        c += tile_part[2 * j + 1];
    }
    block_sum2(a, c);
    if (threadIdx.x == 0) {
        state[0] = a;
        state[1] = c;
    }
}

// init and load: plan the chunk split of all rows into the workspace, prepare, reduce
template <bool INIT>
int pagerank_start(const char* name, const int64_t* rowptr, int64_t num_nodes, int64_t num_edges, const int32_t* out_degree, float* x,
                   float* y, float* inv_out, float* state, void* workspace, size_t workspace_bytes, sage_stream_t stream) {
    SAGE_REQUIRE(num_nodes >= 1 && num_nodes < (1ll << 31), "%s: num_nodes = %lld", name, (long long)num_nodes);
    SAGE_REQUIRE(num_edges >= 0, "%s: num_edges = %lld", name, (long long)num_edges);
    PrLayout L;
    SAGE_REQUIRE(pr_layout(num_nodes, num_edges, &L), "%s: num_nodes = %lld, num_edges = %lld out of range", name, (long long)num_nodes,
                 (long long)num_edges);
    SAGE_REQUIRE(rowptr && x && y && inv_out && state, "%s: NULL array", name);
    SAGE_REQUIRE(x != y && x != inv_out && y != inv_out, "%s: x, y and inv_out must be three arrays", name);
    if (const int rc = csr_workspace_check(name, workspace, workspace_bytes, L.total)) return rc;
    hipStream_t st = (hipStream_t)stream;
    ChunkPlan P;
    if (const int rc = csr_chunk_plan(rowptr, num_nodes, nullptr, (int)num_nodes, workspace, L.c, st, &P)) return rc;
    float* tile_part = (float*)((char*)workspace + L.tile_part);
    hipLaunchKernelGGL(pagerank_prepare_kernel<INIT>, dim3((unsigned)L.tiles), dim3(kPrThreads), 0, st, rowptr, num_nodes, out_degree, x, y, inv_out,
                       tile_part);
    SAGE_CHECK_LAUNCH("pagerank_prepare_kernel");
    hipLaunchKernelGGL(pagerank_reduce_kernel, dim3(1), dim3(kPrThreads), 0, st, (const float*)tile_part, L.tiles, state);
    SAGE_CHECK_LAUNCH("pagerank_reduce_kernel");
    return SAGE_OK;
}

}  // namespace

extern "C" size_t sage_pagerank_workspace_bytes(int64_t num_nodes, int64_t num_edges) {
    PrLayout L;
    return pr_layout(num_nodes, num_edges, &L) ? L.total : 0;
}

extern "C" int sage_pagerank_init(const int64_t* rowptr, int64_t num_nodes, int64_t num_edges, const int32_t* out_degree, float* x, float* y,
                                  float* inv_out, float* state, void* workspace, size_t workspace_bytes, sage_stream_t stream) {
    return pagerank_start<true>("pagerank_init", rowptr, num_nodes, num_edges, out_degree, x, y, inv_out, state, workspace, workspace_bytes,
                                stream);
}

extern "C" int sage_pagerank_load(const int64_t* rowptr, int64_t num_nodes, int64_t num_edges, const float* x, const float* inv_out, float* y,
                                  float* state, void* workspace, size_t workspace_bytes, sage_stream_t stream) {
    // the prepare kernel's <false> form reads x and inv_out and writes neither
    return pagerank_start<false>("pagerank_load", rowptr, num_nodes, num_edges, nullptr, const_cast<float*>(x), y, const_cast<float*>(inv_out),
                                 state, workspace, workspace_bytes, stream);
}

extern "C" int sage_pagerank_step(const int64_t* rowptr, const int32_t* col, int64_t num_nodes, int64_t num_edges, const float* inv_out,
                                  float alpha, const float* x, const float* y, float* x_next, float* y_next, float* state, void* workspace,
                                  size_t workspace_bytes, sage_stream_t stream) {
    SAGE_REQUIRE(num_nodes >= 1 && num_nodes < (1ll << 31), "pagerank_step: num_nodes = %lld", (long long)num_nodes);
    SAGE_REQUIRE(num_edges >= 0, "pagerank_step: num_edges = %lld", (long long)num_edges);
    SAGE_REQUIRE(alpha > 0.f && alpha < 1.f, "pagerank_step: alpha = %g, expected inside (0, 1)", (double)alpha);
    PrLayout L;
    SAGE_REQUIRE(pr_layout(num_nodes, num_edges, &L), "pagerank_step: num_nodes = %lld, num_edges = %lld out of range", (long long)num_nodes,
                 (long long)num_edges);
    SAGE_REQUIRE(rowptr && col && inv_out && x && y && x_next && y_next && state, "pagerank_step: NULL array");
    SAGE_REQUIRE(x_next != x && x_next != y && x_next != inv_out && y_next != x && y_next != y && y_next != inv_out && x_next != y_next,
                 "pagerank_step: x_next and y_next must be arrays of their own (ping-pong buffers)");
    if (const int rc = csr_workspace_check("pagerank_step", workspace, workspace_bytes, L.total)) return rc;
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace;
    const ChunkPlan P{(int64_t*)(ws + L.c.off), (int64_t*)(ws + L.c.carry), (int32_t*)(ws + L.c.item_row), (float*)(ws + L.c.partials), L.c.cap,
                      (int)L.c.nblocks};
    float* tile_part = (float*)(ws + L.tile_part);
    if (P.cap > 0) {
        const int blocks = (int)std::min<int64_t>((P.cap + kPrGroups - 1) / kPrGroups, kNumCU * 8);
        hipLaunchKernelGGL(pagerank_chunk_kernel, dim3(blocks), dim3(kPrThreads), 0, st, rowptr, col, num_nodes, y, (const int64_t*)P.off,
                           (const int64_t*)P.carry, P.nb, P.cap, (const int32_t*)P.item_row, P.partials);
        SAGE_CHECK_LAUNCH("pagerank_chunk_kernel");
    }
    hipLaunchKernelGGL(pagerank_step_kernel, dim3((unsigned)L.tiles), dim3(kPrThreads), 0, st, rowptr, col, num_nodes, inv_out, alpha, x, y, x_next,
                       y_next, (const float*)state, (const int64_t*)P.off, P.cap, (const float*)P.partials, tile_part);
    SAGE_CHECK_LAUNCH("pagerank_step_kernel");
    hipLaunchKernelGGL(pagerank_reduce_kernel, dim3(1), dim3(kPrThreads), 0, st, (const float*)tile_part, L.tiles, state);
    SAGE_CHECK_LAUNCH("pagerank_reduce_kernel");
    return SAGE_OK;
}
