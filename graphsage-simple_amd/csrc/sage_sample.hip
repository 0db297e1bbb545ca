// Fixed-fanout neighbour sampler + frontier (distinct-id) construction.
//
// Replaces, for one hop (include/sage355.h cites the same lines):
//   encoders.py:47          to_neighs = [adj_lists[int(n)] for n in nodes]
//   aggregators.py:42-48    k distinct uniform neighbours, or all if deg < k
//   aggregators.py:52-53    unique_nodes_list / unique_nodes (frontier + id->row)
//
// Shape of the work: tiny and latency bound (B*k2 = 1e5 ids, |S1|*k1 = 3.5e5 ids at
// BASELINE config 3) -- integer work, a chain of dependent HBM round trips per node
// (rowptr -> col -> hash CAS).  A GROUP of G = 8/16/32/64 lanes owns one node and lane i
// owns sample slot i, so every memory step of the chain is one wave-wide instruction
// (k col reads, k hash CAS in flight at once); a first version with one thread per node
// serialised its k CAS round trips and took 52 us for 4096 seeds.  Floyd's subset
// algorithm is inherently sequential in i, but each step only asks "is t_i among the
// i positions already chosen": one group-wide compare + ballot, so the k steps cost
// ~8 instructions each for the whole group.  Frontier rows are reserved per BLOCK
// (wave ballot -> LDS counter -> one global atomic per block): a single counter word
// saturates at ~88 atomics/us on this part.
#include "sage_sample_body.h"

namespace {

using namespace sage_sample_detail;

template <int G, int THREADS, bool SAMPLE, bool FRONTIER>
__global__ __launch_bounds__(THREADS) void sample_kernel(
    const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col,
    const int32_t* __restrict__ nodes, int n, const int32_t* __restrict__ n_dev,
    int k, uint32_t key0, uint32_t key1, uint32_t tag, int tag_self_rows, uint32_t tag_self,
    const int32_t* __restrict__ in_nbr, const int32_t* __restrict__ in_cnt,
    int32_t* __restrict__ nbr, int32_t* __restrict__ cnt, int32_t* __restrict__ any_nonempty,
    FrontierDev f, int insert_self, int32_t* __restrict__ nbr_slot, int32_t* __restrict__ self_slot, BatchSrc bs,
    int n_off, ResolveJob rj) {
    sample_block<G, THREADS, SAMPLE, FRONTIER>(rowptr, col, nodes, n, n_dev, k, key0, key1, tag, tag_self_rows, tag_self, in_nbr, in_cnt, nbr, cnt,
                                               any_nonempty, f, insert_self, nbr_slot, self_slot, bs, n_off, rj, (int)blockIdx.x, (int)gridDim.x);
}

// Outer hop + frontier + inner hop in ONE launch, no grid-wide barrier: the inner hop needs no frontier of its own
// (layer-1 neighbour sets are not deduplicated, aggregators.py:52 works per call), only the ROW its node got, and a block
// knows the rows of the ids it was first to insert as soon as its own counter add returns.  So each block samples the
// outer neighbours of its seeds, inserts them, and then walks the ids it won (LDS list) with lane groups of G1, drawing
// their inner neighbours into nbr1 / cnt1 at those rows; the concat encoder's seed rows (second enc1 call, encoders.py:49-52)
// are drawn by the block that owns the seeds.  What the inner-hop launch used to do besides -- translate the outer hop's hash
// SLOTS into frontier ROWS and wipe the used keys -- has moved into the layer-2 kernel, the only consumer of the rows.
// VERDICT r1 #1 ("merge outer+inner sample (+resolve) into one launch").  Measured: 24.3 us against 10.3 + 11.4 us + a boundary for the
// two launches -- a block's winners (~185 of its 800 ids) take three dependent rounds of its 64 lane groups where the separate inner
// launch spreads 23.6 k nodes over 1500 blocks in one round -- and 66.8 vs 66.2 us per forward in the role pipeline.  Kept as a
// tested option (SAGE_SAMPLE_FUSED=1); the default stays two launches.
template <int G2, int G1, int THREADS>
__global__ __launch_bounds__(THREADS) void sample_fused_kernel(
    const int64_t* __restrict__ rowptr2, const int32_t* __restrict__ col2, const int64_t* __restrict__ rowptr1, const int32_t* __restrict__ col1,
    const int32_t* __restrict__ nodes, int n, int k2, int k1, uint32_t key0, uint32_t key1,
    int32_t* __restrict__ nbr2, int32_t* __restrict__ cnt2, int32_t* __restrict__ any2, FrontierDev f, int insert_self,
    int32_t* __restrict__ nbr_slot, int32_t* __restrict__ self_slot, BatchSrc bs,
    int32_t* __restrict__ nbr1, int32_t* __restrict__ cnt1, int32_t* __restrict__ any1, int seed_rows) {
    constexpr int GPB2 = THREADS / G2;
    __shared__ int32_t wl_ids[THREADS + GPB2];
    __shared__ int32_t wl_seeds[GPB2];
    __shared__ int wl_count, wl_base, blk_any1;
    __shared__ uint32_t wl_key[2];
    const WinList wl{wl_ids, &wl_count, &wl_base, wl_seeds, wl_key};
    if (threadIdx.x == 0) { wl_count = 0; wl_base = 0; blk_any1 = 0; }
    sample_block<G2, THREADS, true, true>(rowptr2, col2, nodes, n, nullptr, k2, key0, key1, SAGE_TAG_OUTER, 0, SAGE_TAG_OUTER, nullptr, nullptr,
                                          nbr2, cnt2, any2, f, insert_self, nbr_slot, self_slot, bs, 0, ResolveJob{}, (int)blockIdx.x,
                                          (int)gridDim.x, wl);
    __syncthreads();
    const uint32_t q0 = wl_key[0], q1 = wl_key[1];
    bool any = false;
    sample_inner_items<G1, THREADS>(rowptr1, col1, bs.num_nodes, wl_ids, wl_count, wl_base, f.max_nodes, k1, q0, q1, SAGE_TAG_INNER, nbr1, cnt1, any);
    if (seed_rows) {
        const int r0 = (int)blockIdx.x * GPB2;
        sample_inner_items<G1, THREADS>(rowptr1, col1, bs.num_nodes, wl_seeds, min(GPB2, n - r0), r0, seed_rows, k1, q0, q1, SAGE_TAG_INNER_SELF,
                                        nbr1, cnt1, any);
    }
    if (any1) {
        if (__any(any) && (threadIdx.x & (kWave - 1)) == 0) blk_any1 = 1;
        __syncthreads();
        if (threadIdx.x == 0 && blk_any1 && *any1 == 0) *any1 = 1;
    }
}

__global__ void frontier_reset_kernel(int32_t* __restrict__ keys, int cap, int32_t* __restrict__ count, int first_row) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int stride = gridDim.x * blockDim.x;
    // cap is a power of two >= 4 and keys is 16-byte aligned (host-checked)
    int4* k4 = reinterpret_cast<int4*>(keys);
    for (int q = i; q < cap / 4; q += stride) k4[q] = make_int4(-1, -1, -1, -1);
    if (i == 0) *count = first_row;
}

int check_frontier(const sage_frontier_t* f, int64_t inserts) {
    SAGE_REQUIRE(f->keys && f->rows && f->nodes && f->count, "frontier: NULL member");
    SAGE_REQUIRE(f->capacity >= 4 && (f->capacity & (f->capacity - 1)) == 0, "frontier: capacity %d not a power of two >= 4", f->capacity);
    SAGE_REQUIRE((int64_t)f->capacity >= 2 * inserts, "frontier: capacity %d < 2 x %lld possible ids", f->capacity, (long long)inserts);
    SAGE_REQUIRE(f->max_nodes > 0, "frontier: max_nodes %d", f->max_nodes);
    SAGE_REQUIRE(sage_aligned(f->keys, 16), "frontier: keys not 16-byte aligned");
    return SAGE_OK;
}

// A sampler kernel and the launch shape that goes with it (nodes per block = threads / G)
using sample_kernel_t = decltype(&sample_kernel<8, 256, true, false>);
struct SampleLaunch { sample_kernel_t kernel; int threads; int nodes_per_block; };

template <int T, bool SAMPLE, bool FRONTIER>
SampleLaunch pick_by_fanout_t(int k) {
    if (k <= 8) return {sample_kernel<8, T, SAMPLE, FRONTIER>, T, T / 8};
    if (k <= 16) return {sample_kernel<16, T, SAMPLE, FRONTIER>, T, T / 16};
    if (k <= 32) return {sample_kernel<32, T, SAMPLE, FRONTIER>, T, T / 32};
    return {sample_kernel<64, T, SAMPLE, FRONTIER>, T, T / 64};
}

template <bool SAMPLE, bool FRONTIER>
SampleLaunch pick_by_fanout(int k) {
    // frontier variants use 1024-thread blocks: one global counter atomic per 1024/G nodes (256- and 512-thread
    // blocks were measured 3-5 % slower end to end)
    if constexpr (FRONTIER) {
        const int so = sage_tunables().outer_threads;
        if (so == 256) return pick_by_fanout_t<256, SAMPLE, FRONTIER>(k);
        if (so == 512) return pick_by_fanout_t<512, SAMPLE, FRONTIER>(k);
        return pick_by_fanout_t<1024, SAMPLE, FRONTIER>(k);
    }
#ifndef SAGE_SI_THREADS
#define SAGE_SI_THREADS 256
#endif
    else return pick_by_fanout_t<SAGE_SI_THREADS, SAMPLE, FRONTIER>(k);
}

}  // namespace

int sage_check_frontier(const sage_frontier_t* f, int64_t inserts) { return check_frontier(f, inserts); }

// Internal launcher shared with sage_forward.hip (sage_sample_t: sage_internal.h)
int sage_launch_sample(const sage_sample_t& s, hipStream_t st, sage_launch_events_t* ev) {
    if (s.n == 0) return SAGE_OK;
    const sage_model_t* qm = s.queue_model;
    const BatchSrc bs{qm ? qm->queue : nullptr, qm ? qm->queue_cursor : nullptr, qm ? qm->queue_len : 0, s.nodes_from_batch, s.nodes_copy,
                      (qm && s.nodes_from_batch) ? qm->seed_map : s.seed_map, (int)s.num_nodes};
    ResolveJob rj{};
    if (const sage_resolve_t* r = s.resolve)
        rj = ResolveJob{r->slots, r->rows_out, r->n_slots, r->self_slots, r->self_rows_out, r->n_self, r->hash_rows, r->hash_keys};
    FrontierDev fd{};
    if (const sage_frontier_t* f = s.frontier)
        fd = FrontierDev{f->keys, f->rows, (uint32_t)f->capacity - 1u, f->nodes, f->count, f->max_nodes, s.frontier_row_off};
    const SampleLaunch L = s.frontier ? pick_by_fanout<true, true>(s.k) : pick_by_fanout<true, false>(s.k);
    const int32_t* none = nullptr;
    sage_launch(L.kernel, dim3(sage_cdiv(s.n, L.nodes_per_block)), dim3(L.threads), 0, st, ev, s.rowptr, s.col, s.nodes, s.n, s.n_dev, s.k,
                (uint32_t)s.seed, (uint32_t)(s.seed >> 32), s.tag, s.tag_self_rows, s.tag_self, none, none, s.nbr, s.cnt, s.any_nonempty, fd,
                s.frontier ? s.insert_self : 0, s.frontier ? s.nbr_slot : nullptr, s.frontier ? s.self_slot : nullptr, bs, s.n_off, rj);
    SAGE_CHECK_LAUNCH("sample_kernel");
    return SAGE_OK;
}

namespace {
using sample_fused_kernel_t = decltype(&sample_fused_kernel<16, 16, 512>);
struct FusedSampleLaunch { sample_fused_kernel_t kernel; int threads; int seeds_per_block; };

template <int G2, int G1>
FusedSampleLaunch pick_fused_by_threads() {
    if (sage_tunables().outer_threads >= 1024) return {sample_fused_kernel<G2, G1, 1024>, 1024, 1024 / G2};
    return {sample_fused_kernel<G2, G1, 512>, 512, 512 / G2};
}
template <int G2>
FusedSampleLaunch pick_fused_by_k1(int k1) {
    if (k1 <= 16) return pick_fused_by_threads<G2, 16>();
    if (k1 <= 32) return pick_fused_by_threads<G2, 32>();
    return pick_fused_by_threads<G2, 64>();
}
}  // namespace

int sage_launch_sample_fused(const sage_sample_fused_t& s, hipStream_t st) {
    if (s.batch == 0) return SAGE_OK;
    const sage_model_t* m = s.m;
    const BatchSrc bs{s.queued ? m->queue : nullptr, s.queued ? m->queue_cursor : nullptr, s.queued ? m->queue_len : 0, 1, s.nodes_copy,
                      m->seed_map, (int)m->num_nodes};
    const sage_frontier_t* f = s.frontier;
    const FrontierDev fd{f->keys, f->rows, (uint32_t)f->capacity - 1u, f->nodes, f->count, f->max_nodes, s.frontier_row_off};
    const FusedSampleLaunch L = m->k2 <= 16 ? pick_fused_by_k1<16>(m->k1) : m->k2 <= 32 ? pick_fused_by_k1<32>(m->k1) : pick_fused_by_k1<64>(m->k1);
    hipLaunchKernelGGL(L.kernel, dim3(sage_cdiv(s.batch, L.seeds_per_block)), dim3(L.threads), 0, st, m->rowptr2, m->col2, m->rowptr1, m->col1,
                       s.seeds, s.batch, m->k2, m->k1, (uint32_t)s.seed, (uint32_t)(s.seed >> 32), s.nbr2, s.cnt2, s.any2, fd, s.insert_self,
                       s.nbr_slot, s.self_slot, bs, s.nbr1, s.cnt1, s.any1, s.seed_rows);
    SAGE_CHECK_LAUNCH("sample_fused_kernel");
    return SAGE_OK;
}

extern "C" int sage_frontier_reset(const sage_frontier_t* f, int32_t first_row, sage_stream_t stream) {
    SAGE_REQUIRE(f, "frontier_reset: NULL frontier");
    if (int rc = check_frontier(f, 0)) return rc;
    SAGE_REQUIRE(first_row >= 0 && first_row <= f->max_nodes, "frontier_reset: first_row %d outside [0, %d]", first_row, f->max_nodes);
    const int blocks = min(sage_cdiv(f->capacity / 4, 256), 1024);
    hipLaunchKernelGGL(frontier_reset_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, f->keys, f->capacity, f->count, first_row);
    SAGE_CHECK_LAUNCH("frontier_reset_kernel");
    return SAGE_OK;
}

extern "C" int sage_sample_neighbors(const int64_t* rowptr, const int32_t* col, int64_t num_nodes, const int32_t* nodes,
                                     int32_t n, const int32_t* n_dev, int32_t k, uint64_t seed, uint32_t tag, int32_t* nbr,
                                     int32_t* cnt, int32_t* any_nonempty, const sage_frontier_t* frontier, int32_t insert_self,
                                     int32_t* nbr_slot, int32_t* self_slot, sage_stream_t stream) {
    SAGE_REQUIRE(rowptr && col && nodes && nbr && cnt, "sample_neighbors: NULL array");
    SAGE_REQUIRE(n >= 0, "sample_neighbors: n = %d", n);
    SAGE_REQUIRE(k >= 1 && k <= SAGE_MAX_FANOUT, "sample_neighbors: k = %d outside [1, %d]", k, SAGE_MAX_FANOUT);
    SAGE_REQUIRE(num_nodes > 0 && num_nodes < (1ll << 31), "sample_neighbors: num_nodes = %lld", (long long)num_nodes);
    if (frontier) {
        if (int rc = check_frontier(frontier, (int64_t)n * (k + (insert_self ? 1 : 0)))) return rc;
        SAGE_REQUIRE(nbr_slot, "sample_neighbors: frontier given but nbr_slot is NULL");
        SAGE_REQUIRE(!insert_self || self_slot, "sample_neighbors: insert_self needs self_slot");
    }
    return sage_launch_sample({.rowptr = rowptr, .col = col, .num_nodes = num_nodes, .nodes = nodes, .n = n, .n_dev = n_dev, .k = k, .seed = seed,
                               .tag = tag, .tag_self = tag, .nbr = nbr, .cnt = cnt, .any_nonempty = any_nonempty, .frontier = frontier,
                               .insert_self = insert_self, .nbr_slot = nbr_slot, .self_slot = self_slot},
                              (hipStream_t)stream);
}

extern "C" int sage_frontier_insert(const int32_t* nbr, const int32_t* cnt, int32_t k, const int32_t* self_nodes, int32_t n,
                                    const int32_t* n_dev, const sage_frontier_t* frontier, int32_t* nbr_slot, int32_t* self_slot,
                                    sage_stream_t stream) {
    SAGE_REQUIRE(nbr && cnt && frontier && nbr_slot, "frontier_insert: NULL array");
    SAGE_REQUIRE(n >= 0, "frontier_insert: n = %d", n);
    SAGE_REQUIRE(k >= 1 && k <= SAGE_MAX_FANOUT, "frontier_insert: k = %d outside [1, %d]", k, SAGE_MAX_FANOUT);
    SAGE_REQUIRE(!self_nodes || self_slot, "frontier_insert: self_nodes needs self_slot");
    if (int rc = check_frontier(frontier, (int64_t)n * (k + (self_nodes ? 1 : 0)))) return rc;
    if (n == 0) return SAGE_OK;
    const FrontierDev fd{frontier->keys, frontier->rows, (uint32_t)frontier->capacity - 1u,
                         frontier->nodes, frontier->count, frontier->max_nodes, 0};
    const int64_t* no64 = nullptr;
    const int32_t* no32 = nullptr;
    const SampleLaunch L = pick_by_fanout<false, true>(k);
    hipLaunchKernelGGL(L.kernel, dim3(sage_cdiv(n, L.nodes_per_block)), dim3(L.threads), 0, (hipStream_t)stream, no64, no32, self_nodes, n, n_dev, k,
                       0u, 0u, 0u, 0, 0u, nbr, cnt, (int32_t*)nullptr, (int32_t*)nullptr, (int32_t*)nullptr, fd, self_nodes ? 1 : 0, nbr_slot,
                       self_slot, BatchSrc{nullptr, nullptr, 0, 0, nullptr, nullptr, 0}, 0, ResolveJob{});
    SAGE_CHECK_LAUNCH("frontier_insert_kernel");
    return SAGE_OK;
}
