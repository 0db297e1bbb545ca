// Internal (non-ABI) launchers shared between translation units of libsage355.
#pragma once
#include "sage_common.h"

// forward2 plumbing shared by the launchers -------------------------------------------------
struct sage_resolve_t {          // see ResolveJob in sage_sample.hip
    const int32_t* slots; int32_t* rows_out; int32_t n_slots;
    const int32_t* self_slots; int32_t* self_rows_out; int32_t n_self;
    const int32_t* hash_rows; int32_t* hash_keys;
};
// With the fused sampler the layer-2 kernel receives hash SLOTS (nbr, self_row) and turns them into frontier rows itself
// (slot_rows = the hash's rows array); on the way it wipes the keys it reads (which leaves the table clean for the next forward) and
// leaves the rows in rows_out / self_rows_out for read-back (tests, the training step's backward).
struct sage_slot_resolve_t {
    int32_t* wipe_keys;          // [capacity] hash keys; keys[slot] := -1 for every slot read
    int32_t* rows_out;           // [n, k]  frontier row of every neighbour slot (-1 = padding)
    int32_t* self_rows_out;      // nullable [n]
};
// The LAST kernel of a forward: its last-finishing block zeroes the forward's device counters
// (counters[0..6]; counters[7] is the ticket) and advances the batch-queue cursor, so the next
// forward needs no memset / reset / advance launches.
struct sage_finish_t {
    int32_t* counters;           // nullable = no finish duty
    int32_t* cursor;             // nullable
};
// What the launchers take ------------------------------------------------------------------
// Plain aggregates, filled at the call site by member name (designated initialisers, which hipcc accepts under -std=c++17);
// every nullable / optional member defaults to "absent".
//
// The rows a launch reads: a row-major table (row stride ld), or a slice-major one ([dim / ld][table_rows][ld], slice_stride =
// table_rows * ld floats between slices; ld IS the slice width then).
struct sage_rows_t {
    const float* table; int64_t table_rows; int64_t ld; int32_t dim;
    int64_t slice_stride = 0;
};
// The n destination rows of a launch and their neighbour lists.  Device-side row count = min(*n_dev + n_off, n).  A launch that
// reads finished means instead of lists (sage_launch_layer_dense, sage_launch_linear_act) uses n, n_dev and n_off only.
struct sage_lists_t {
    const int32_t* nbr = nullptr;            // [n, k] ids of table rows (hash slots with slot_rows), -1 = padding
    const int32_t* cnt = nullptr;            // [n]
    int32_t k = 0;
    int32_t n;
    const int32_t* n_dev = nullptr; int32_t n_off = 0;
    const int32_t* slot_rows = nullptr;      // ids in nbr / self_row are slots of this array
    const int32_t* self_row = nullptr;       // [n] the row's own id joins its set (aggregators.py:50-51)
    const int32_t* any_nonempty = nullptr;   // the reference's 0/0 = NaN rule for empty rows applies when *any_nonempty != 0
};
// Concat encoder: where a destination row's own features come from (row self_index[r], or r).  self_tab == NULL: no concat.
struct sage_self_t {
    const float* self_tab = nullptr; int64_t ld_self = 0; int64_t self_rows = 0; const int32_t* self_index = nullptr;
};
// out = act([self |] mean . weight^T)
struct sage_contract_t {
    const float* weight; int64_t ldw; const void* weight_prepared = nullptr;      // (sage_prepare_weights)
    int32_t out_dim; int32_t act; float* out; int64_t ldo;
};

// The events one launch is to carry as ITS OWN start / stop events (the two slots of hipExtLaunchKernelGGL), passed by the caller to
// the launcher of the kernel that is to carry them; `carried` is set by sage_launch when the launch really did (a launcher's n == 0
// early return, or a form of it that does not take events, leaves it false).
//   {nullptr, tail}: a tail event.  A stage's hand-off event rides on the stage's LAST kernel as that dispatch's own completion signal
//       instead of being a packet of its own behind the kernel (hipEventRecord): one barrier packet less between two kernels of a role
//       stream (experiments/r04/handoff.hip: 7.3 against 8.5 us per hand-off; in the pipeline the record was one of the two packets
//       that separate consecutive kernels of a stream).  Where it was not carried the caller records it (sage_forward.hip).
//   {start, stop}: the measurement pair (bench.py's dominant-kernel duration): two TIMING events around the layer-1 gather launch,
//       i.e. the interval is the kernel's execution (what rocprofv3 reports) and not the distance between two marker packets around
//       it in a busy queue.  Only the stop slot can hold a tail, so a launch that carries the pair cannot carry a tail as well.
// Never while a stream is capturing (hipExtLaunchKernel is not a capturable launch).
struct sage_launch_events_t { void* start = nullptr; void* stop = nullptr; bool carried = false; };
#ifdef __HIPCC__
#include <hip/hip_ext.h>
// One kernel launch: plain, or with `e`'s events as the launch's own
template <class... P, class... A>
void sage_launch(void (*kernel)(P...), dim3 grid, dim3 block, size_t lds, hipStream_t st, sage_launch_events_t* e, A&&... a) {
    if (e && (e->start || e->stop)) {
        hipExtLaunchKernelGGL(kernel, grid, block, lds, st, (hipEvent_t)e->start, (hipEvent_t)e->stop, 0u, static_cast<P>(a)...);
        e->carried = true;
    } else {
        hipLaunchKernelGGL(kernel, grid, block, lds, st, static_cast<P>(a)...);
    }
}
#endif

// One sampling hop (sage_sample.hip).  Rows [0, tag_self_rows) draw from stream `tag_self` (the concat encoder's second enc1 call on
// the seeds); with `frontier` the sampled ids are inserted and get rows from frontier_row_off on.
struct sage_sample_t {
    const int64_t* rowptr; const int32_t* col; int64_t num_nodes;
    const int32_t* nodes; int32_t n; const int32_t* n_dev = nullptr; int32_t n_off = 0;
    int32_t k; uint64_t seed; uint32_t tag; int32_t tag_self_rows = 0; uint32_t tag_self = 0;
    int32_t* nbr; int32_t* cnt; int32_t* any_nonempty = nullptr;
    const sage_frontier_t* frontier = nullptr; int32_t frontier_row_off = 0; int32_t insert_self = 0;
    int32_t* nbr_slot = nullptr; int32_t* self_slot = nullptr;
    const sage_model_t* queue_model = nullptr;     // seeds (nodes_from_batch) and sampler key come from the model's batch queue
    int nodes_from_batch = 0;
    int32_t* nodes_copy = nullptr;                 // nodes[r] (internal id) is also written here
    const int32_t* seed_map = nullptr;             // nodes[r] is a caller id
    const sage_resolve_t* resolve = nullptr;
};
int sage_launch_sample(const sage_sample_t& s, hipStream_t st, sage_launch_events_t* ev = nullptr);
// The same hop for k up to SAGE_MAX_FANOUT_WIDE, one wave per node (sage_sample_wide.hip).  Takes the members of a plain call only:
// a batch queue, seed map, resolve job, row offset or second tag is refused (SAGE_EINVAL).
int sage_launch_sample_wide(const sage_sample_t& s, hipStream_t st);
// Host check of a frontier that is about to take up to `inserts` ids (sage_sample.hip)
int sage_check_frontier(const sage_frontier_t* f, int64_t inserts);

// Both hops of a forward as one launch (see sample_fused_kernel).  `seed_rows` = batch for the concat encoder (rows [0, batch) of
// S1 are the seeds themselves), else 0.
struct sage_sample_fused_t {
    const sage_model_t* m; const int32_t* seeds; int32_t batch; uint64_t seed; int queued = 0;
    int32_t* nbr2; int32_t* cnt2; int32_t* any2 = nullptr;
    const sage_frontier_t* frontier; int32_t frontier_row_off = 0; int32_t insert_self = 0; int32_t* nbr_slot; int32_t* self_slot = nullptr;
    int32_t* nodes_copy = nullptr;
    int32_t* nbr1; int32_t* cnt1; int32_t* any1 = nullptr; int32_t seed_rows = 0;
};
int sage_launch_sample_fused(const sage_sample_fused_t& s, hipStream_t st);

// `act` exists in the column-sliced forms only, and only they carry `ev`
int sage_launch_gather_mean(const sage_rows_t& src, const sage_lists_t& l, float* out, int64_t ldo, int32_t act, hipStream_t st,
                            sage_launch_events_t* ev = nullptr);
bool sage_layer_dense_supported(int32_t dim, int32_t out_dim);
bool sage_gather_is_sliced(int32_t dim, int64_t ld, int64_t ldo, const float* table, const float* out, int32_t n, int32_t k);

int sage_launch_linear_act(const sage_rows_t& agg, const sage_lists_t& rows, const sage_self_t& self, const sage_contract_t& c,
                           sage_finish_t fin, hipStream_t st);

// Fused layer (sage_fused.hip).  Returns SAGE_EUNSUPPORTED when no instantiation fits.  `self` must name the source table (SAGE_EINVAL).
// `company`: what other batches run on the chip while this launch does, as far as the caller knows -- it picks the block shape of the
// small-layer (tile16) form, never the arithmetic: every shape returns the same bits.
enum sage_layer_company_t {
    SAGE_BESIDE_ANYTHING = 0,             // unknown, or persistent kernels that share their CUs (column-sliced gather, contraction): 512-thread blocks
    SAGE_BESIDE_ONE_WAVE_LAYER1 = 1,      // the phase-sliced layer 1 of the next batch, one wave of blocks that fills every CU: 1024-thread blocks
    SAGE_BESIDE_LAYER1_AND_INNER_SAMPLER = 2,   // the same with every batch's inner sampler in that layer 1's queue, in front of it (role pipeline,
                                          // sage_pipe.hip round 11): 512-thread blocks again -- measured there: 51.6 us per forward against 65.7
};
int sage_launch_layer_fused(const sage_rows_t& src, const sage_lists_t& l, const sage_self_t& self, const sage_contract_t& c,
                            const sage_slot_resolve_t* resolve, sage_finish_t fin, hipStream_t st, sage_launch_events_t* ev = nullptr,
                            sage_layer_company_t company = SAGE_BESIDE_ANYTHING);
bool sage_layer_fused_supported(int32_t dim, int32_t out_dim, int32_t concat);
int sage_launch_layer_dense(const sage_rows_t& agg, const sage_lists_t& rows, const sage_self_t& self, const sage_contract_t& c,
                            sage_finish_t fin, hipStream_t st, sage_launch_events_t* ev = nullptr);

// Phase-sliced layer 1 (sage_layer1_phase.hip): gather + contraction of the gcn encoder's layer 1 in one launch on the slice-major table
// of 32-float slices, bit-identical to sage_launch_gather_mean + sage_launch_layer_dense.  SAGE_EUNSUPPORTED when the shape has no kernel.
bool sage_layer1_phase_supported(int32_t d0, int32_t h1, int32_t k);
int sage_launch_layer1_phase(const sage_rows_t& src, const sage_lists_t& l, const sage_contract_t& c, hipStream_t st,
                             sage_launch_events_t* ev = nullptr);

// Classifier head (sage_head.hip): scores, cross-entropy and its gradients of one batch.  The row kernel takes this struct by value.
// part_w / part_loss: the per-range partials in the caller's workspace ([ranges][C * dim] and [ranges]); part_w == NULL: no weight
// gradient.  The launcher runs the fixed-order reduce into grad_w / loss when either is asked for.  Arguments are validated by the caller.
struct sage_head_t {
    const float* emb; int64_t lde; int32_t dim;
    const float* w_cls; int64_t ldw; int32_t num_classes;
    const int64_t* labels = nullptr; int32_t n; float scale = 1.f;
    float* scores = nullptr; int64_t lds = 0; int32_t* pred = nullptr;
    float* grad_emb = nullptr; int64_t ldg = 0;
    float* part_w = nullptr; float* part_loss = nullptr;
    float* grad_w = nullptr; int64_t ldgw = 0; float* loss = nullptr;
};
int sage_launch_xent_head(const sage_head_t& h, hipStream_t st);

// The launches of one forward, by stage (sage_pipe.hip enqueues each stage on its role stream)
#define SAGE_STAGE_SAMPLE_OUTER 1
#define SAGE_STAGE_SAMPLE_INNER 2
#define SAGE_STAGE_GATHER1      4
#define SAGE_STAGE_CONTRACT1    8     /* whole layer 1 when it is a one-launch layer */
#define SAGE_STAGE_LAYER2       16
#define SAGE_STAGE_ALL          31
int sage_forward2_launch_stages(const sage_model_t* m, void* workspace, size_t workspace_bytes, const int32_t* seeds, int32_t batch,
                                uint64_t seed, float* out, int64_t ldo, int32_t stages, hipStream_t stream, void* tail_event = nullptr,
                                void* const* gather_events = nullptr, bool inner_with_layer1 = false);

bool sage_forward2_contract1_is_empty(const sage_model_t* m, int32_t batch);
bool sage_forward2_sampler_is_fused(const sage_model_t* m);

// Launch-shape tunables, read ONCE from the environment (A/B runs on one box without rebuilding; defaults are the
// measured optima recorded in DESIGN.md).  Every value is clamped to a safe range.
struct sage_tunables_t {
    int gather_blocks_per_cu;     // SAGE_G_PER_CU        sliced gather: 256-thread blocks per CU (1..8), default 6
    int gather_slice_lanes;       // SAGE_G_SLICE_LANES   0 = by row width (16 lanes = 256-B slices; 32 for narrow odd rows), or 8 / 16 / 32 / 64 (64: variant 1 only)
    int gather_rows_in_flight;    // SAGE_G_ROWS          pipelined gather: rows of a wave in flight together (1 / 2 / 4), default 1
    int gather_trip;              // SAGE_G_TRIP          rows form: neighbours of a row requested per trip (8 / 16), default 16
    int gather_variant;           // SAGE_G_VARIANT       0 = three-trip rows, 1 = rows software-pipelined (default), 2 = one row per lane group
    int gather_variant_sliced;    // SAGE_G_VARIANT_SM    the variant used with a slice-major table (sage_model_t.table_sliced): 2 (default) / 1 / 0
    int dense_blocks;             // SAGE_DENSE_BLOCKS    split-bf16 contraction: persistent 512-thread blocks (32..512), default 224
    int bwd_blocks;               // SAGE_BWD_BLOCKS      weight-gradient GEMM: blocks over (tiles x K splits), default 2 per CU (every split adds its tile with fp32 atomics)
    int bwd_direct_blocks;        // SAGE_BWD_DIRECT_BLOCKS  reproducible weight gradient: row ranges = 512-thread blocks = partial tiles (16..1024), default 256
    int outer_threads;            // SAGE_SO_THREADS      outer-hop sampler block size (256 / 512 / 1024), default 512 (1024 until round 3)
    int tile16_grid;              // SAGE_T16_GRID        layer-2 tile16 kernel: max blocks (64..1024), default 512
    int sample_fused;             // SAGE_SAMPLE_FUSED    1: both hops in one launch when layer 2 is a one-launch layer; 0 (default): two launches
                                  //                      (measured: 24.3 us fused vs 10.3 + 11.4: the inner hop of a block's own winners is
                                  //                      three dependent rounds on 128-256 blocks instead of one round on 1500; pipeline 66.8 vs 66.2 us)
    int tile16_waves;             // SAGE_T16_WAVES       layer-2 tile16 kernel: 16 (1024-thread blocks) or 8 (512-thread blocks); 0 (default, unset) = by the
                                  //                      launch's company, sage_layer_company_t: 16 beside the one-launch layer 1 alone, 8 otherwise
    int tile16_inflight;          // SAGE_T16_INFLIGHT    layer-2 tile16 kernel, gcn form with 16 waves: 7 or 13 row loads of a lane group in flight per trip
                                  //                      (13: the 25-entry list of config 3 in ONE trip); 0 (default, unset) = by the launch's company:
                                  //                      13 beside the one-launch layer 1, 7 otherwise.  Every other form has 7
    int layer1_fused;             // SAGE_LAYER1_FUSED    1: layer 1 as ONE phase-sliced launch where its conditions hold and nobody needs the means
                                  //                      (sage_layer1_phase.hip); 0: always gather + contraction.  Default: see sage_api.hip
    int layer1_phase_tiles;       // SAGE_L1P_TILES       phase-sliced layer 1: 32-row tiles a block walks in ping-pong, 2 (default) or 1
    int layer1_phase_per_cu;      // SAGE_L1P_PER_CU      phase-sliced layer 1: persistent 256-thread blocks per CU: 1..2 with two tiles per
                                  //                      block (default 2), 1..3 with one (default 3)
};
// n_words 32-bit words := v, as a kernel (hipMemsetAsync misbehaves inside replayed hipGraphs on ROCm 7.2: sage_api.hip)
int sage_fill_u32(void* p, uint32_t v, size_t n_words, hipStream_t st);
const sage_tunables_t& sage_tunables();

// Narrowest layer that takes the split form (column-sliced gather + dense contraction) instead of the one-launch layer.
#ifndef SAGE_SPLIT_MIN_DIM
#define SAGE_SPLIT_MIN_DIM 64
#endif

#ifdef __HIPCC__
// Finish duty of the forward's last kernel: the block that draws the last ticket zeroes the counters (keeping a
// read-back copy for tests / byte counting) and advances the batch-queue cursor.  Split in two so that the loads
// the duty needs are in flight while the block does its real work: sage_finish_begin() at kernel start (thread 0;
// the counters are final before this kernel starts), sage_finish_block() by EVERY block after its last use of them.
struct sage_finish_regs { int32_t c[7]; int32_t cur; };

__device__ inline void sage_finish_begin(const sage_finish_t& fin, sage_finish_regs& r) {
    if (!fin.counters || threadIdx.x != 0) return;
#pragma unroll
    for (int i = 0; i < 7; ++i) r.c[i] = fin.counters[i];
    r.cur = fin.cursor ? *fin.cursor : 0;
}

__device__ inline void sage_finish_block(const sage_finish_t& fin, int total_blocks, const sage_finish_regs& r) {
    if (!fin.counters) return;
    __syncthreads();
    if (threadIdx.x == 0) {
        // No __threadfence() here: on gfx950 it is `buffer_wbl2 sc1` + `buffer_inv sc1` -- a write-back and an
        // invalidate of the XCD's whole L2, once per block, which also throws out the other batch's cached hub rows
        // (measured: layer 2 16.7 -> 10.7 us alone, forward 98 -> 90 us with two batches in flight).
        // It is not needed: every block has consumed the counters it read (its row count decides its whole loop)
        // before the barrier above, the ticket is taken after that barrier, and the block that draws the last ticket
        // is the only writer; the kernel boundary publishes its stores to the next launch.
        if (__hip_atomic_fetch_add(&fin.counters[7], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == total_blocks - 1) {
#pragma unroll
            for (int i = 0; i < 7; ++i) {
                fin.counters[8 + i] = r.c[i];             // read-back copy (tests, byte counting)
                fin.counters[i] = 0;
            }
            fin.counters[7] = 0;
            if (fin.cursor) *fin.cursor = r.cur + 1;
        }
    }
}

// one-call form (kernels whose blocks have nothing to overlap the loads with)
__device__ inline void sage_finish_block(const sage_finish_t& fin, int total_blocks) {
    sage_finish_regs r;
    sage_finish_begin(fin, r);
    sage_finish_block(fin, total_blocks, r);
}
#endif
