// Two-layer ("2-hop") forward: graphsage/model.py:219-222 wiring of two Encoders,
// enqueued on one stream with no host synchronisation.
//
//   seeds --sample k2 (enc2.adj)--> nbr2 --hash--> frontier U2 = layer-1 node list S1
//   S1    --sample k1 (enc1.adj)--> nbr1
//   layer 1 on S1 : h1 = act1( [table[S1] |] mean(table[nbr1]) . W1^T )     (encoders.py:47-62)
//   layer 2 on B  : out = act2( [h1[seed] |] mean(h1[row(nbr2)]) . W2^T )
//
// Concat encoder (gcn=False): the reference evaluates layer 1 a SECOND time on the seeds
// (self_feats = features(nodes), encoders.py:49-52) with samples of its own; those B rows
// sit at the head of S1 (rows [0,B)) and draw from RNG stream SAGE_TAG_INNER_SELF, the
// frontier rows follow from row B.
#include <string.h>

#include "sage_internal.h"

namespace {

size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

int next_pow2(int64_t x) {
    int64_t p = 4;
    while (p < x) p <<= 1;
    return (int)p;
}

int check_model(const sage_model_t* m) {
    SAGE_REQUIRE(m, "forward2: NULL model");
    SAGE_REQUIRE(m->num_nodes > 0 && m->num_nodes < (1ll << 31), "forward2: num_nodes = %lld", (long long)m->num_nodes);
    SAGE_REQUIRE(m->d0 >= 1 && m->h1 >= 1 && m->h2 >= 1, "forward2: dims d0=%d h1=%d h2=%d", m->d0, m->h1, m->h2);
    SAGE_REQUIRE(m->k1 >= 1 && m->k1 <= SAGE_MAX_FANOUT && m->k2 >= 1 && m->k2 <= SAGE_MAX_FANOUT,
                 "forward2: fanouts k1=%d k2=%d outside [1, %d]", m->k1, m->k2, SAGE_MAX_FANOUT);
    SAGE_REQUIRE(m->table_ld >= m->d0, "forward2: table_ld = %lld < d0", (long long)m->table_ld);
    SAGE_REQUIRE(m->act1 >= 0 && m->act1 <= SAGE_ACT_NONE && m->act2 >= 0 && m->act2 <= SAGE_ACT_NONE, "forward2: bad activation");
    return SAGE_OK;
}

}  // namespace

extern "C" int sage_forward2_layout(const sage_model_t* m, int32_t max_batch, sage_ws_layout_t* L) {
    if (int rc = check_model(m)) return rc;
    SAGE_REQUIRE(L, "forward2_layout: NULL layout");
    SAGE_REQUIRE(max_batch >= 1 && (int64_t)max_batch * (m->k2 + 1) < (1ll << 30), "forward2_layout: max_batch = %d", max_batch);
    memset(L, 0, sizeof(*L));
    const int64_t B = max_batch;
    const int64_t max_s1 = B * m->k2 + B;   // frontier of B*k2 ids + B self rows (concat or self-loop)
    size_t off = 0;
    auto take = [&](size_t bytes) { size_t o = off; off = align_up(off + bytes, 256); return o; };
    L->counters = take(32 * sizeof(int32_t));    // 16 counters in use; the rest of the 32 is padding that keeps the offsets the Python layer reads
    L->hash_capacity = next_pow2(2 * B * (m->k2 + 1));
    L->hash_keys = take((size_t)L->hash_capacity * 4);
    L->hash_rows = take((size_t)L->hash_capacity * 4);
    L->max_s1 = (int32_t)max_s1;
    L->s1_nodes = take((size_t)max_s1 * 4);
    L->nbr2 = take((size_t)B * m->k2 * 4);
    L->slot2 = take((size_t)B * m->k2 * 4);
    L->cnt2 = take((size_t)B * 4);
    L->self_slot2 = take((size_t)B * 4);
    L->row2 = take((size_t)B * m->k2 * 4);
    L->self_row2 = take((size_t)B * 4);
    L->nbr1 = take((size_t)max_s1 * m->k1 * 4);
    L->cnt1 = take((size_t)max_s1 * 4);
    L->agg1 = take((size_t)max_s1 * m->d0 * 4);
    L->h1 = take((size_t)max_s1 * m->h1 * 4);
    L->agg2 = take((size_t)B * m->h1 * 4);
    L->total_bytes = off;
    L->layer1_split = (m->fused && sage_layer_dense_supported(m->d0, m->h1) && m->table_ld % 4 == 0 && m->k1 <= 64 &&
                       ((m->d0 >= SAGE_SPLIT_MIN_DIM && max_s1 >= 8192) || m->d0 > 256)) ? 1 : 0;
#ifdef SAGE_FORCE_FUSED1
    L->layer1_split = 0;
#endif
    return SAGE_OK;
}

namespace {
// ev: NULL, or 2*SAGE_NUM_STAGES hipEvent_t (begin, end per stage; NULL entries skipped)
#define SAGE_EV(i)                                                                         \
    do {                                                                                   \
        if (ev && ev[i] && hipEventRecord((hipEvent_t)ev[i], st) != hipSuccess) {          \
            sage_set_error("forward2: hipEventRecord failed");                             \
            return SAGE_ELAUNCH;                                                           \
        }                                                                                  \
    } while (0)

// Which launches layer 1 is made of (a function of the model and the layout only, so every call on a workspace -- and the role pipeline,
// which must know whether its D stage launches anything -- agrees)
struct layer1_form_t {
    bool split1;          // wide + large layer 1: column-sliced gather (cross-XCD L2 partitioning) into agg1, then a dense contraction
    bool gather_only1;    // serving on a pre-transformed table (sage_model_t.w1_is_identity): the split layer's gather applies act1 and writes h1
    bool phase1;          // the split layer 1 as ONE phase-sliced launch (sage_layer1_phase.hip; bit-identical h1): gcn encoder, slice-major table of
                          // 32-float slices, prepared W1, and nobody needs the means (sage_model_t.keep_means: the backward reads agg1)
};
layer1_form_t layer1_form(const sage_model_t* m, const sage_ws_layout_t& L, const float* agg1, const float* h1) {
    layer1_form_t f;
    f.split1 = m->fused && L.layer1_split && sage_aligned(m->table, 16) && sage_aligned(m->w1, 16) &&
               sage_gather_is_sliced(m->d0, m->table_ld, m->d0, m->table, agg1, L.max_s1, m->k1);
    f.gather_only1 = f.split1 && m->w1_is_identity != 0 && !m->concat && m->d0 == m->h1 &&
                     sage_gather_is_sliced(m->d0, m->table_ld, m->h1, m->table, h1, L.max_s1, m->k1);
    f.phase1 = f.split1 && !f.gather_only1 && !m->concat && !m->keep_means && sage_tunables().layer1_fused != 0 &&
               m->table_sliced != nullptr && m->table_slice_floats == 32 && sage_aligned(m->table_sliced, 16) &&
               m->w1_prepared != nullptr && sage_layer1_phase_supported(m->d0, m->h1, m->k1);
    return f;
}

bool layer2_is_fused(const sage_model_t* m) {
    return m->fused && sage_layer_fused_supported(m->h1, m->h2, m->concat) && sage_aligned(m->w2, 16);
}
}  // namespace

// Both hops are sampled by ONE launch for this model: the two sampling stages cannot be enqueued apart (the role pipeline asks)
bool sage_forward2_sampler_is_fused(const sage_model_t* m) {
    return layer2_is_fused(m) && sage_tunables().sample_fused != 0 && m->k1 <= 64 && m->k2 <= 64;
}

namespace {
int forward2_impl(const sage_model_t* m, void* workspace, size_t workspace_bytes, const int32_t* seeds, int32_t batch,
                  uint64_t seed, float* out, int64_t ldo, sage_stream_t stream, void* const* ev, int stages = SAGE_STAGE_ALL,
                  void* tail_event = nullptr, void* const* gather_events = nullptr, bool inner_with_layer1 = false) {
    if (int rc = check_model(m)) return rc;
    SAGE_REQUIRE(m->rowptr1 && m->col1 && m->rowptr2 && m->col2 && m->table && m->w1 && m->w2, "forward2: NULL model array");
    const bool queued = m->queue != nullptr;
    SAGE_REQUIRE(!queued || (m->queue_len >= 1 && m->queue_cursor), "forward2: batch queue without length / cursor");
    SAGE_REQUIRE(workspace && (seeds || queued) && (out || !(stages & SAGE_STAGE_LAYER2)), "forward2: NULL argument");
    SAGE_REQUIRE(batch >= 1, "forward2: batch = %d", batch);
    SAGE_REQUIRE(ldo >= m->h2 || !(stages & SAGE_STAGE_LAYER2), "forward2: ldo = %lld < h2", (long long)ldo);
    SAGE_REQUIRE(sage_aligned(workspace, 256), "forward2: workspace not 256-byte aligned");
    SAGE_REQUIRE(m->ws_batch == 0 || batch <= m->ws_batch, "forward2: batch %d > ws_batch %d", batch, m->ws_batch);
    sage_ws_layout_t L;
    if (int rc = sage_forward2_layout(m, m->ws_batch ? m->ws_batch : batch, &L)) return rc;
    if (L.total_bytes > workspace_bytes) {
        sage_set_error("forward2: workspace %zu bytes < %zu needed for batch %d", workspace_bytes, L.total_bytes, batch);
        return SAGE_ENOSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    // tail_event (sage_pipe.hip): to be recorded behind the LAST launch of `stages` -- as that launch's own completion signal where its
    // launcher takes events, by hipEventRecord otherwise (run_stage below)
    int last_stage = 0;
    for (int bit = SAGE_STAGE_LAYER2; bit >= 1; bit >>= 1)
        if (tail_event && (stages & bit)) { last_stage = bit; break; }
    char* ws = (char*)workspace;
    int32_t* counters = (int32_t*)(ws + L.counters);
    int32_t* s1_count = counters + 0;      // frontier rows claimed so far (zero based; rows start at first_row)
    int32_t* any2 = counters + 1;
    int32_t* any1 = counters + 2;
    int32_t* s1_nodes = (int32_t*)(ws + L.s1_nodes);
    int32_t* nbr2 = (int32_t*)(ws + L.nbr2);
    int32_t* slot2 = (int32_t*)(ws + L.slot2);
    int32_t* cnt2 = (int32_t*)(ws + L.cnt2);
    int32_t* self_slot2 = (int32_t*)(ws + L.self_slot2);
    int32_t* row2 = (int32_t*)(ws + L.row2);
    int32_t* self_row2 = (int32_t*)(ws + L.self_row2);
    int32_t* nbr1 = (int32_t*)(ws + L.nbr1);
    int32_t* cnt1 = (int32_t*)(ws + L.cnt1);
    float* agg1 = (float*)(ws + L.agg1);
    float* h1 = (float*)(ws + L.h1);
    float* agg2 = (float*)(ws + L.agg2);
    const sage_frontier_t fr{(int32_t*)(ws + L.hash_keys), (int32_t*)(ws + L.hash_rows), L.hash_capacity, s1_nodes, s1_count, L.max_s1};
    const int first_row = m->concat ? batch : 0;
    const int self_loop = m->agg_self_loop ? 1 : 0;
    const sage_model_t* qm = queued ? m : nullptr;
    const sage_finish_t no_fin{nullptr, nullptr};
    const sage_finish_t fin{counters, queued ? m->queue_cursor : nullptr};

    // The workspace is self-cleaning (sage_forward2_init once, then every forward leaves the hash
    // keys wiped and the counters zero), so a forward is exactly 4 launches (5 when layer 1 is split into
    // gather + contraction, 6 with the generic two-launch layers).
    const bool fuse1 = m->fused && sage_layer_fused_supported(m->d0, m->h1, m->concat) && m->table_ld % 4 == 0 &&
                       sage_aligned(m->table, 16) && sage_aligned(m->w1, 16);
    // wide + large layer 1: column-sliced gather into agg1, then a dense contraction (or both in one phase-sliced launch);
    // otherwise the one-launch fused layer; otherwise the generic two-launch form
    const layer1_form_t form1 = layer1_form(m, L, agg1, h1);
    const bool split1 = form1.split1, gather_only1 = form1.gather_only1, phase1 = form1.phase1;
    // Layer 2 as a one-launch layer resolves hash slots itself, so both hops can be sampled by ONE launch (sage_sample.hip:
    // sample_fused_kernel).  The choice depends on the model only, so every call on a workspace agrees on who resolves the slots.
    const bool fuse2 = layer2_is_fused(m);
    const bool sfused = sage_forward2_sampler_is_fused(m);

    // What the launches below read and write, each described once.
    // Layer 1: rows [0, s1_count + first_row) of S1 gather from the feature table ...
    const sage_rows_t table1{.table = m->table, .table_rows = m->num_nodes, .ld = m->table_ld, .dim = m->d0};
    // ... or, in the column-sliced forms, from its optional slice-major copy ([d0 / sw][num_nodes][sw]: every XCD pair reads ONE contiguous array)
    const int sw = m->table_slice_floats ? m->table_slice_floats : 64;
    const bool sm = m->table_sliced != nullptr && (sw == 32 || sw == 64 || sw == 128) && m->d0 % sw == 0 && sage_aligned(m->table_sliced, 16);
    const sage_rows_t table1_sliced = !sm ? table1 : sage_rows_t{.table = m->table_sliced, .table_rows = m->num_nodes, .ld = sw, .dim = m->d0,
                                                                 .slice_stride = m->num_nodes * (int64_t)sw};
    const sage_lists_t lists1{.nbr = nbr1, .cnt = cnt1, .k = m->k1, .n = L.max_s1, .n_dev = s1_count, .n_off = first_row,
                              .self_row = self_loop ? s1_nodes : nullptr, .any_nonempty = m->nan_empty ? any1 : nullptr};
    const sage_rows_t means1{.table = agg1, .table_rows = L.max_s1, .ld = m->d0, .dim = m->d0};
    const sage_self_t self1{.self_tab = m->concat ? m->table : nullptr, .ld_self = m->table_ld, .self_rows = m->num_nodes, .self_index = s1_nodes};
    const sage_contract_t contract1{.weight = m->w1, .ldw = (int64_t)m->d0 * (m->concat ? 2 : 1), .weight_prepared = m->w1_prepared,
                                    .out_dim = m->h1, .act = m->act1, .out = h1, .ldo = m->h1};
    // Layer 2: the seeds gather from h1, by frontier row -- or by hash slot when the fused sampler left the slots unresolved: the layer
    // then resolves them (rows left in row2 / self_row2) and wipes the keys, the duties the inner-hop launch has otherwise.
    // Outer hop: some neighbour was sampled  <=>  the frontier counter is non-zero, so layer 2 needs no flag at all
    const int32_t* nan2 = m->nan_empty ? (self_loop ? any2 : s1_count) : nullptr;
    const sage_rows_t table2{.table = h1, .table_rows = L.max_s1, .ld = m->h1, .dim = m->h1};
    const sage_lists_t lists2 = sfused ? sage_lists_t{.nbr = slot2, .cnt = cnt2, .k = m->k2, .n = batch, .slot_rows = fr.rows,
                                                      .self_row = self_loop ? self_slot2 : nullptr, .any_nonempty = nan2}
                                       : sage_lists_t{.nbr = row2, .cnt = cnt2, .k = m->k2, .n = batch,
                                                      .self_row = self_loop ? self_row2 : nullptr, .any_nonempty = nan2};
    const sage_slot_resolve_t resolve2{fr.keys, row2, self_loop ? self_row2 : nullptr};
    const sage_rows_t means2{.table = agg2, .table_rows = batch, .ld = m->h1, .dim = m->h1};
    const sage_self_t self2{.self_tab = m->concat ? h1 : nullptr, .ld_self = m->h1, .self_rows = L.max_s1};
    const sage_contract_t contract2{.weight = m->w2, .ldw = (int64_t)m->h1 * (m->concat ? 2 : 1), .out_dim = m->h2, .act = m->act2, .out = out,
                                    .ldo = ldo};

    // One stage: body(e) makes the stage's launches and hands e to the launcher of the LAST one.  e holds the events that launch is to
    // carry: `own` (the gather's measurement pair, which replaces the stage's marker events) when given, otherwise the tail when this is
    // the last requested stage, otherwise nothing.  A tail that did not ride -- the stage launched nothing, its last launcher takes no
    // events or returned early, or the launch carried the measurement pair -- is recorded behind the stage.  Profiled forward: marker
    // events `first` and `first + 1` around the stage.
    auto run_stage = [&](int stage, int first, const sage_launch_events_t* own, auto body) -> int {
        const bool tail_here = (stage & last_stage) != 0;
        sage_launch_events_t e = own ? *own : tail_here ? sage_launch_events_t{nullptr, tail_event} : sage_launch_events_t{};
        if (!own) SAGE_EV(first);
        if (int rc = body(&e)) return rc;
        if (tail_here && !(e.carried && !own) && hipEventRecord((hipEvent_t)tail_event, st) != hipSuccess) {
            sage_set_error("forward2: hipEventRecord failed");
            return SAGE_ELAUNCH;
        }
        if (!own) SAGE_EV(first + 1);
        return SAGE_OK;
    };

    const int both = SAGE_STAGE_SAMPLE_OUTER | SAGE_STAGE_SAMPLE_INNER;
    if (sfused && (stages & both)) {
        SAGE_REQUIRE((stages & both) == both, "forward2: with the fused sampler the two sampling stages are one launch: pass "
                                                "SAGE_STAGE_SAMPLE_OUTER | SAGE_STAGE_SAMPLE_INNER together");
        // (event 0 before the one launch, events 1 to 3 behind it)
        if (int rc = run_stage(both, 0, nullptr, [&](sage_launch_events_t*) {
                return sage_launch_sample_fused({.m = m, .seeds = seeds, .batch = batch, .seed = seed, .queued = queued ? 1 : 0,
                                                 .nbr2 = nbr2, .cnt2 = cnt2, .any2 = (m->nan_empty && self_loop) ? any2 : nullptr,
                                                 .frontier = &fr, .frontier_row_off = first_row, .insert_self = self_loop, .nbr_slot = slot2,
                                                 .self_slot = self_slot2, .nodes_copy = m->concat ? s1_nodes : nullptr,
                                                 .nbr1 = nbr1, .cnt1 = cnt1, .any1 = m->nan_empty ? any1 : nullptr,
                                                 .seed_rows = first_row /* = batch for the concat encoder, else 0 */}, st);
            }))
            return rc;
        SAGE_EV(2);
        SAGE_EV(3);
    }
    // 1. outer hop: seeds -> nbr2, hash insert -> frontier rows [first_row, ...)
    if (!sfused && (stages & SAGE_STAGE_SAMPLE_OUTER))
        if (int rc = run_stage(SAGE_STAGE_SAMPLE_OUTER, 0, nullptr, [&](sage_launch_events_t* e) {
                return sage_launch_sample({.rowptr = m->rowptr2, .col = m->col2, .num_nodes = m->num_nodes, .nodes = seeds, .n = batch,
                                           .k = m->k2, .seed = seed, .tag = SAGE_TAG_OUTER, .tag_self = SAGE_TAG_OUTER,
                                           .nbr = nbr2, .cnt = cnt2, .any_nonempty = (m->nan_empty && self_loop) ? any2 : nullptr,
                                           .frontier = &fr, .frontier_row_off = first_row, .insert_self = self_loop, .nbr_slot = slot2,
                                           .self_slot = self_slot2, .queue_model = qm, .nodes_from_batch = 1,
                                           .nodes_copy = m->concat ? s1_nodes : nullptr, .seed_map = m->seed_map}, st, e);
            }))
            return rc;
    // 2. inner hop: S1 -> nbr1 (raw table rows; duplicates are served by L2 / Infinity Cache).  Its spare
    //    threads turn the outer hop's hash slots into frontier rows and wipe the used keys.
    //    (Drawing these samples inside the layer-1 gather instead was measured: the gather went from 48 to
    //    100 us, its per-row dependent chain growing from 2 to 5 round trips.)
    if (!sfused && (stages & SAGE_STAGE_SAMPLE_INNER))
        if (int rc = run_stage(SAGE_STAGE_SAMPLE_INNER, 2, nullptr, [&](sage_launch_events_t* e) {
                const sage_resolve_t resolve{slot2, row2, batch * m->k2, self_loop ? self_slot2 : nullptr, self_row2, batch, fr.rows, fr.keys};
                return sage_launch_sample({.rowptr = m->rowptr1, .col = m->col1, .num_nodes = m->num_nodes, .nodes = s1_nodes, .n = L.max_s1,
                                           .n_dev = s1_count, .n_off = first_row, .k = m->k1, .seed = seed, .tag = SAGE_TAG_INNER,
                                           .tag_self_rows = first_row, .tag_self = SAGE_TAG_INNER_SELF,
                                           .nbr = nbr1, .cnt = cnt1, .any_nonempty = m->nan_empty ? any1 : nullptr, .queue_model = qm,
                                           .resolve = &resolve}, st, e);
            }))
            return rc;
    // 3. layer 1 on S1: the HBM-bound gather (nothing when layer 1 is a one-launch or a generic layer) ...
    if (stages & SAGE_STAGE_GATHER1) {
        // The measurement pair, as the gather launch's own start / stop events when it takes a column-sliced or the phase-sliced form:
        // the caller's (sage_pipe_submit_profiled), or events 4 / 5 of sage_forward2_profiled, which are marker records otherwise
        sage_launch_events_t pair;
        if (gather_events) pair = {gather_events[0], gather_events[1]};
        else if (ev && (gather_only1 || split1)) pair = {ev[4], ev[5]};
        if (int rc = run_stage(SAGE_STAGE_GATHER1, 4, pair.start && pair.stop ? &pair : nullptr, [&](sage_launch_events_t* e) {
                if (phase1) return sage_launch_layer1_phase(table1_sliced, lists1, contract1, st, e);
                if (split1)      // means into agg1 -- or, on a pre-transformed table (gather_only1), activated and straight into h1
                    return sage_launch_gather_mean(table1_sliced, lists1, gather_only1 ? h1 : agg1, gather_only1 ? m->h1 : m->d0,
                                                   gather_only1 ? m->act1 : SAGE_ACT_NONE, st, e);
                return (int)SAGE_OK;
            }))
            return rc;
    }
    // ... and its contraction (one launch with the gather unless the layer is split; nothing when the gather stage wrote h1)
    if (stages & SAGE_STAGE_CONTRACT1)
        if (int rc = run_stage(SAGE_STAGE_CONTRACT1, 6, nullptr, [&](sage_launch_events_t* e) {
                if (gather_only1 || phase1) return (int)SAGE_OK;
                if (split1) return sage_launch_layer_dense(means1, lists1, self1, contract1, no_fin, st, e);
                if (fuse1) return sage_launch_layer_fused(table1, lists1, self1, contract1, nullptr, no_fin, st, e);
                if (int rc = sage_launch_gather_mean(table1, lists1, agg1, m->d0, SAGE_ACT_NONE, st)) return rc;
                return sage_launch_linear_act(means1, lists1, self1, contract1, no_fin, st);
            }))
            return rc;
    // 4. layer 2 on the seeds; its last block zeroes the counters and advances the batch queue
    if (stages & SAGE_STAGE_LAYER2)
        if (int rc = run_stage(SAGE_STAGE_LAYER2, 8, nullptr, [&](sage_launch_events_t* e) {
                // in a pipeline this launch runs beside the NEXT batch's layer 1: the block shape follows that kernel's form (sage_fused.hip)
                if (fuse2) return sage_launch_layer_fused(table2, lists2, self2, contract2, sfused ? &resolve2 : nullptr, fin, st, e,
                                                          !phase1 ? SAGE_BESIDE_ANYTHING : inner_with_layer1 ? SAGE_BESIDE_LAYER1_AND_INNER_SAMPLER
                                                                                                             : SAGE_BESIDE_ONE_WAVE_LAYER1);
                if (int rc = sage_launch_gather_mean(table2, lists2, agg2, m->h1, SAGE_ACT_NONE, st)) return rc;
                return sage_launch_linear_act(means2, lists2, self2, contract2, fin, st);
            }))
            return rc;
    return SAGE_OK;
}
}  // namespace

extern "C" int sage_forward2(const sage_model_t* m, void* workspace, size_t workspace_bytes, const int32_t* seeds, int32_t batch,
                             uint64_t seed, float* out, int64_t ldo, sage_stream_t stream) {
    return forward2_impl(m, workspace, workspace_bytes, seeds, batch, seed, out, ldo, stream, nullptr);
}

// SAGE_STAGE_CONTRACT1 launches nothing for this model (the gather stage writes h1): the role pipeline then skips stage D's hand-off
bool sage_forward2_contract1_is_empty(const sage_model_t* m, int32_t batch) {
    sage_ws_layout_t L;
    if (check_model(m) != SAGE_OK || sage_forward2_layout(m, m->ws_batch ? m->ws_batch : batch, &L) != SAGE_OK) return false;
    const float* aligned = reinterpret_cast<const float*>(uintptr_t{256});      // workspace arrays are 256-byte aligned (forward2_impl requires it)
    const layer1_form_t f = layer1_form(m, L, aligned, aligned);
    return f.gather_only1 || f.phase1;
}

// A subset of the forward's launches with the seeds and the sampler key taken from the call (sage_pipe.hip: one call per role stream)
int sage_forward2_launch_stages(const sage_model_t* m, void* workspace, size_t workspace_bytes, const int32_t* seeds, int32_t batch,
                                uint64_t seed, float* out, int64_t ldo, int32_t stages, hipStream_t stream, void* tail_event,
                                void* const* gather_events, bool inner_with_layer1) {
    // inner_with_layer1: the caller enqueues this batch's inner sampler in front of its layer 1, in one queue (it decides layer 2's company)
    return forward2_impl(m, workspace, workspace_bytes, seeds, batch, seed, out, ldo, (sage_stream_t)stream, nullptr, stages, tail_event,
                         gather_events, inner_with_layer1);
}

extern "C" int sage_forward2_profiled(const sage_model_t* m, void* workspace, size_t workspace_bytes, const int32_t* seeds,
                                      int32_t batch, uint64_t seed, float* out, int64_t ldo, sage_stream_t stream,
                                      void* const* stage_events) {
    return forward2_impl(m, workspace, workspace_bytes, seeds, batch, seed, out, ldo, stream, stage_events);
}

// Put a fresh (or dirty) workspace into the state every forward leaves behind: counters zero,
// hash keys empty.  Call once after allocating the workspace (and after an aborted stream).
extern "C" int sage_forward2_init(const sage_model_t* m, void* workspace, size_t workspace_bytes, int32_t max_batch,
                                  sage_stream_t stream) {
    if (int rc = check_model(m)) return rc;
    SAGE_REQUIRE(workspace && sage_aligned(workspace, 256), "forward2_init: workspace NULL or not 256-byte aligned");
    sage_ws_layout_t L;
    if (int rc = sage_forward2_layout(m, max_batch, &L)) return rc;
    if (L.total_bytes > workspace_bytes) {
        sage_set_error("forward2_init: workspace %zu bytes < %zu needed for batch %d", workspace_bytes, L.total_bytes, max_batch);
        return SAGE_ENOSPACE;
    }
    char* ws = (char*)workspace;
    hipStream_t st = (hipStream_t)stream;
    // smaller batches use a prefix of the key array with a smaller power-of-two capacity: wipe the largest
    if (int rc = sage_fill_u32(ws + L.counters, 0u, 16, st)) return rc;
    if (int rc = sage_fill_u32(ws + L.hash_keys, 0xFFFFFFFFu, (size_t)L.hash_capacity, st)) return rc;
    return SAGE_OK;
}
