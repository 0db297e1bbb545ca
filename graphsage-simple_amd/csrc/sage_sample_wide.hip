// Fixed-fanout neighbour sampler for fanouts above SAGE_MAX_FANOUT, up to SAGE_MAX_FANOUT_WIDE (+ frontier construction).
//
// Replaces, for one hop, the same lines as sage_sample.hip:
//   encoders.py:47          to_neighs = [adj_lists[int(n)] for n in nodes]
//   aggregators.py:42-48    k distinct uniform neighbours, or all if deg < k   (any num_sample: the reference has no limit)
//   aggregators.py:52-53    unique_nodes_list / unique_nodes (frontier + id->row)
//
// The narrow kernel gives one lane to each sample slot, which ends at k = 64.  Here ONE WAVE owns a node and lane l owns the
// slots l, l + 64, l + 128, ... (SPL = slots per lane, 1 .. 16), each in a register of its own: every register array below is
// indexed by compile-time constants once the loops over SPL are unrolled (zero scratch in every instantiation).
//   * the draws: all k Philox words are computed up front, SPL per lane, in parallel;
//   * Floyd's walk stays sequential in i (oracle/sampler_ref.c): step i = 64 q + li reads t_i from lane li's register q
//     (v_readlane), compares it with every pick already made -- registers 0 .. q-1 of every lane and register q of the lanes
//     below li -- and one ballot decides whether lane li keeps t_i or takes j_i.  k steps of q + 4 instructions;
//   * col reads and nbr / nbr_slot writes go in chunks of 64 consecutive slots (coalesced);
//   * frontier: per chunk every lane inserts its id with a global CAS (sage_hash_insert), the wave ballots the winners and
//     reserves their rows with ONE atomicAdd on the counter.  The narrow kernel's block-wide LDS dedupe is left out: a wave here
//     issues one counter atomic per 64 ids as that kernel's block does per ~1000, but the rows of a wide hop are few.
// The draw is the narrow kernel's bit for bit (for k <= 64 the outputs are identical), and a pure function of (seed, tag, v).
#include "sage_internal.h"

namespace {

constexpr int kWideThreads = 256;                       // 4 waves = 4 nodes per block
constexpr int kWideNodesPerBlock = kWideThreads / kWave;

struct WideFrontier {
    int32_t* keys; int32_t* rows; uint32_t mask; int32_t* nodes; int32_t* count; int32_t max_nodes;
};

// Steps i = 64 Q .. min(k, 64 Q + 64) - 1 of Floyd's walk, then the next chunk.  chosen[q] starts as t (the draw) and is final for every
// slot below i.
template <int Q, int SPL>
__device__ __forceinline__ void floyd_chunk(uint32_t (&chosen)[SPL], const uint32_t (&ji)[SPL], int k, int lane) {
    if (64 * Q >= k) return;                            // wave-uniform
    const int steps = min(k - 64 * Q, 64);
    for (int li = (Q == 0 ? 1 : 0); li < steps; ++li) {
        const uint32_t t = (uint32_t)__builtin_amdgcn_readlane((int)chosen[Q], li);
        bool hit = lane < li && chosen[Q] == t;
#pragma unroll
        for (int p = 0; p < Q; ++p) hit |= chosen[p] == t;
        if (__ballot(hit) != 0ull && lane == li) chosen[Q] = ji[Q];
    }
    if constexpr (Q + 1 < SPL) floyd_chunk<Q + 1, SPL>(chosen, ji, k, lane);
}

template <int SPL, bool FRONTIER>
__global__ __launch_bounds__(kWideThreads) void sample_wide_kernel(
    const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col, int num_nodes,
    const int32_t* __restrict__ nodes, int n, const int32_t* __restrict__ n_dev,
    int k, uint32_t key0, uint32_t key1, uint32_t tag,
    int32_t* __restrict__ nbr, int32_t* __restrict__ cnt, int32_t* __restrict__ any_nonempty,
    WideFrontier f, int insert_self, int32_t* __restrict__ nbr_slot, int32_t* __restrict__ self_slot) {
    const int tid = threadIdx.x;
    const int lane = tid & (kWave - 1);
    const int r = (int)blockIdx.x * kWideNodesPerBlock + tid / kWave;
    int nn = n;
    if (n_dev) nn = min(*n_dev, n);
    const bool active = r < nn;                         // wave-uniform, as is everything derived from v below
    int32_t v = -1;
    int64_t s = 0, deg = 0;
    int c = 0;
    if (active) {
        v = nodes[r];
        if ((uint32_t)v < (uint32_t)num_nodes) {        // ids outside [0, num_nodes) are empty rows
            s = rowptr[v];
            deg = rowptr[v + 1] - s;
        }
        c = (int)min(deg, (int64_t)k);
    }
    if (any_nonempty) {
        // one flag word per launch: the block ORs its waves in LDS and thread 0 alone touches the word (see sage_sample_body.h)
        __shared__ int blk_any;
        if (tid == 0) blk_any = 0;
        __syncthreads();
        if (c > 0 && lane == 0) blk_any = 1;
        __syncthreads();
        if (tid == 0 && blk_any && *any_nonempty == 0) *any_nonempty = 1;
    }
    if (!active) return;                                // no barrier below this line

    uint32_t pos[SPL];
#pragma unroll
    for (int q = 0; q < SPL; ++q) pos[q] = (uint32_t)(lane + 64 * q);
    if (deg > (int64_t)k) {
        uint32_t ji[SPL];
#pragma unroll
        for (int q = 0; q < SPL; ++q) {
            const int slot = lane + 64 * q;
            ji[q] = (uint32_t)(deg - (int64_t)k) + (uint32_t)slot;
            uint32_t t = 0;
            if (slot < k) {
                const Philox4 p = philox4x32_10((uint32_t)v, tag, (uint32_t)(slot >> 2), 0u, key0, key1);
                t = sage_bounded(sage_philox_word(p, slot & 3), ji[q] + 1u);
            }
            pos[q] = t;
        }
        floyd_chunk<0, SPL>(pos, ji, k, lane);
    }

    int32_t id[SPL];
#pragma unroll
    for (int q = 0; q < SPL; ++q) {
        const int slot = lane + 64 * q;
        id[q] = -1;
        if (slot < c) id[q] = __builtin_nontemporal_load(col + s + (int64_t)pos[q]);     // pos < deg: Floyd's t <= j < deg, else slot < c <= deg
        if (slot < k) nbr[(int64_t)r * k + slot] = id[q];
    }
    if (lane == 0) cnt[r] = c;

    if constexpr (FRONTIER) {
        const unsigned long long below = (1ull << lane) - 1ull;
        if (insert_self) {
            // v joins the frontier (aggregators.py:50-51 before :52).  A negative id cannot be a key (-1 marks an empty slot).
            bool won = false;
            int sslot = -1;
            if (lane == 0 && v >= 0) sslot = sage_hash_insert(f.keys, f.mask, v, won);
            if (lane == 0) self_slot[r] = sslot;
            if (won) {
                const int row = atomicAdd(f.count, 1);
                if (row < f.max_nodes) f.nodes[row] = v;
                f.rows[sslot] = row;
            }
        }
#pragma unroll
        for (int q = 0; q < SPL; ++q) {
            if (64 * q < k) {                           // wave-uniform
                const int slot = lane + 64 * q;
                bool won = false;
                int hslot = -1;
                if (slot < c) hslot = sage_hash_insert(f.keys, f.mask, id[q], won);
                if (slot < k) nbr_slot[(int64_t)r * k + slot] = hslot;
                const unsigned long long wb = __ballot(won);
                if (wb != 0ull) {
                    int base = 0;
                    if (lane == 0) base = atomicAdd(f.count, __popcll(wb));
                    base = __builtin_amdgcn_readfirstlane(base);
                    if (won) {
                        const int row = base + __popcll(wb & below);
                        if (row < f.max_nodes) f.nodes[row] = id[q];
                        f.rows[hslot] = row;
                    }
                }
            }
        }
    }
}

using sample_wide_kernel_t = decltype(&sample_wide_kernel<1, false>);

template <bool FRONTIER>
sample_wide_kernel_t pick_wide(int k) {
    if (k <= 64) return sample_wide_kernel<1, FRONTIER>;
    if (k <= 128) return sample_wide_kernel<2, FRONTIER>;
    if (k <= 256) return sample_wide_kernel<4, FRONTIER>;
    if (k <= 512) return sample_wide_kernel<8, FRONTIER>;
    return sample_wide_kernel<16, FRONTIER>;
}

}  // namespace

// Internal launcher (sage_sample_t: sage_internal.h).  The wide kernel knows the plain call only: none of forward2's plumbing.
int sage_launch_sample_wide(const sage_sample_t& s, hipStream_t st) {
    SAGE_REQUIRE(s.k >= 1 && s.k <= SAGE_MAX_FANOUT_WIDE, "sample_wide: k = %d outside [1, %d]", s.k, SAGE_MAX_FANOUT_WIDE);
    SAGE_REQUIRE(!s.queue_model && !s.nodes_from_batch && !s.nodes_copy && !s.seed_map && !s.resolve && s.n_off == 0 &&
                     s.tag_self_rows == 0 && s.frontier_row_off == 0,
                 "sample_wide: the wide sampler takes no batch queue, seed map, resolve job, row offset or second tag");
    if (s.n == 0) return SAGE_OK;
    WideFrontier fd{};
    if (const sage_frontier_t* f = s.frontier) fd = WideFrontier{f->keys, f->rows, (uint32_t)f->capacity - 1u, f->nodes, f->count, f->max_nodes};
    const sample_wide_kernel_t kernel = s.frontier ? pick_wide<true>(s.k) : pick_wide<false>(s.k);
    hipLaunchKernelGGL(kernel, dim3(sage_cdiv(s.n, kWideNodesPerBlock)), dim3(kWideThreads), 0, st, s.rowptr, s.col, (int)s.num_nodes, s.nodes,
                       s.n, s.n_dev, s.k, (uint32_t)s.seed, (uint32_t)(s.seed >> 32), s.tag, s.nbr, s.cnt, s.any_nonempty, fd,
                       s.frontier ? s.insert_self : 0, s.frontier ? s.nbr_slot : nullptr, s.frontier ? s.self_slot : nullptr);
    SAGE_CHECK_LAUNCH("sample_wide_kernel");
    return SAGE_OK;
}

extern "C" int sage_sample_neighbors_wide(const int64_t* rowptr, const int32_t* col, int64_t num_nodes, const int32_t* nodes,
                                          int32_t n, const int32_t* n_dev, int32_t k, uint64_t seed, uint32_t tag, int32_t* nbr,
                                          int32_t* cnt, int32_t* any_nonempty, const sage_frontier_t* frontier, int32_t insert_self,
                                          int32_t* nbr_slot, int32_t* self_slot, sage_stream_t stream) {
    SAGE_REQUIRE(rowptr && col && nodes && nbr && cnt, "sample_neighbors_wide: NULL array");
    SAGE_REQUIRE(n >= 0, "sample_neighbors_wide: n = %d", n);
    SAGE_REQUIRE(k >= 1 && k <= SAGE_MAX_FANOUT_WIDE, "sample_neighbors_wide: k = %d outside [1, %d]", k, SAGE_MAX_FANOUT_WIDE);
    SAGE_REQUIRE(num_nodes > 0 && num_nodes < (1ll << 31), "sample_neighbors_wide: num_nodes = %lld", (long long)num_nodes);
    if (frontier) {
        if (int rc = sage_check_frontier(frontier, (int64_t)n * (k + (insert_self ? 1 : 0)))) return rc;
        SAGE_REQUIRE(nbr_slot, "sample_neighbors_wide: frontier given but nbr_slot is NULL");
        SAGE_REQUIRE(!insert_self || self_slot, "sample_neighbors_wide: insert_self needs self_slot");
    }
    return sage_launch_sample_wide({.rowptr = rowptr, .col = col, .num_nodes = num_nodes, .nodes = nodes, .n = n, .n_dev = n_dev, .k = k,
                                    .seed = seed, .tag = tag, .tag_self = tag, .nbr = nbr, .cnt = cnt, .any_nonempty = any_nonempty,
                                    .frontier = frontier, .insert_self = insert_self, .nbr_slot = nbr_slot, .self_slot = self_slot},
                                   (hipStream_t)stream);
}
