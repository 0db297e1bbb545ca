/*
 * sage355.h -- C ABI of libsage355.so: the GraphSAGE sample -> gather -> masked
 * mean -> (concat) -> W.x -> act hot path as hand-written HIP kernels for
 * MI355X (gfx950).
 *
 * The reference (zjzijielu/graphsage-simple) is pure Python and has no FFI;
 * the "operators" of its hot path are the statement groups of
 *   graphsage/aggregators.py:34-76   MeanAggregator.forward
 *   graphsage/encoders.py:40-62      Encoder.forward
 * Each entry point below replaces one such group and cites it.  A maintainer
 * binds them with ctypes (INTEGRATION.md shows the stub); this repo's own host
 * side (graphsage-simple_amd/sage355/) does exactly that.
 *
 * Conventions
 *  - Every pointer is a DEVICE pointer (HBM) unless the name ends in _host.
 *    The library never allocates, frees or synchronises: the caller owns all
 *    memory (so a caching allocator and hipGraph capture both work).
 *  - `stream` is a hipStream_t passed as void* (NULL = the default stream).
 *  - Node ids are int32 (N < 2^31), CSR row pointers int64, features fp32
 *    row-major with an explicit leading dimension in ELEMENTS.
 *  - Row counts come in pairs (n, n_dev): `n` is the host-side upper bound used
 *    to size the launch; if `n_dev` is non-NULL the kernels read the actual
 *    count from it (min(*n_dev, n)), so a frontier whose size is only known on
 *    the device needs no host round trip.
 *  - Return value: SAGE_OK or a negative SAGE_E* code; sage_last_error() gives
 *    the message for the calling thread.  Arguments are validated on the host
 *    BEFORE any launch (an out-of-range kernel access can reset the whole
 *    node), so a call either enqueues all of its kernels or none.
 */
#ifndef SAGE355_H
#define SAGE355_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SAGE_ABI_VERSION 9

#define SAGE_OK            0
#define SAGE_EINVAL       -1   /* bad argument (NULL, size, alignment, range) */
#define SAGE_EUNSUPPORTED -2   /* valid request this build has no kernel for  */
#define SAGE_ELAUNCH      -3   /* hipLaunch / runtime error                   */
#define SAGE_ENOSPACE     -4   /* workspace too small                         */

#define SAGE_ACT_RELU    0     /* encoders.py:61; NaN propagates like torch.relu */
#define SAGE_ACT_SIGMOID 1     /* encoders.py:58-59 (node_degree/shared/pagerank) */
#define SAGE_ACT_NONE    2

#define SAGE_MAX_FANOUT  64    /* device sampler limit on k (BASELINE uses <= 25) */

/* RNG stream tags: which sampling call a draw belongs to (see oracle/sampler_ref.c). */
#define SAGE_TAG_INNER      1  /* layer-1 samples of the frontier            */
#define SAGE_TAG_OUTER      2  /* layer-2 samples of the seeds               */
#define SAGE_TAG_INNER_SELF 3  /* concat encoder: layer-1 samples of the seeds (2nd enc1 call) */

typedef void* sage_stream_t;

int         sage_abi_version(void);
const char* sage_last_error(void);
/* Name of the code-object architecture the library was built for ("gfx950"). */
const char* sage_build_arch(void);

/* ---------------------------------------------------------------------------
 * Frontier: the set of distinct ids one hop produces, plus id -> row lookup.
 * Replaces `unique_nodes_list = list(set.union(*samp_neighs))` and the
 * `unique_nodes` dict (aggregators.py:52-53).  Open-addressing hash in HBM:
 * keys[slot] = node id (or -1), rows[slot] = position of that id in nodes[].
 * The ORDER of nodes[] is arbitrary (as a Python set's is); everything
 * computed from it is order independent.
 * ------------------------------------------------------------------------- */
typedef struct {
    int32_t* keys;        /* [capacity]  -1 = empty; reset with sage_frontier_reset */
    int32_t* rows;        /* [capacity]  row of keys[slot] in nodes[]               */
    int32_t  capacity;    /* power of two, >= 2 * max distinct ids                   */
    int32_t* nodes;       /* [max_nodes] the distinct ids, arbitrary order           */
    int32_t* count;       /* [1] device counter: number of rows in nodes[] so far    */
    int32_t  max_nodes;
} sage_frontier_t;

/* keys[] := -1, *count := first_row (rows below first_row are reserved by the caller). */
int sage_frontier_reset(const sage_frontier_t* f, int32_t first_row, sage_stream_t stream);

/* ---------------------------------------------------------------------------
 * sage_sample_neighbors -- encoders.py:47 (adjacency fetch) + aggregators.py:42-48
 * (fixed-fanout sample) [+ aggregators.py:52-53 when `frontier` is given].
 *
 * For node v = nodes[r], deg = rowptr[v+1]-rowptr[v]:
 *   deg >  k : k DISTINCT uniform positions of the CSR row (Floyd's subset
 *              algorithm, O(k); Philox4x32-10 keyed by `seed`, counter
 *              (v, tag, draw/4)) -> cnt[r] = k
 *   deg <= k : the whole row, in CSR order              -> cnt[r] = deg
 * nbr[r*k + j], j < cnt[r], are global node ids; entries j >= cnt[r] are -1.
 * The draw for (seed, tag, v) does not depend on r, n or the launch shape.
 *
 * frontier != NULL: every sampled id (and v itself when `insert_self`) is
 * inserted; nbr_slot[r*k+j] receives its hash slot and self_slot[r] the slot of
 * v.  rows[slot] is valid once this call's kernels have completed (stream
 * order), so a consumer reads row = frontier->rows[nbr_slot[e]].
 * any_nonempty (nullable): set to 1 if any cnt[r] > 0 (reference NaN rule).
 * Ids outside [0, num_nodes) are empty rows; rows at or past min(*n_dev, n)
 * are not written; a negative v is never inserted; its self_slot is -1.
 * ------------------------------------------------------------------------- */
int sage_sample_neighbors(const int64_t* rowptr, const int32_t* col, int64_t num_nodes,
                          const int32_t* nodes, int32_t n, const int32_t* n_dev,
                          int32_t k, uint64_t seed, uint32_t tag,
                          int32_t* nbr, int32_t* cnt, int32_t* any_nonempty,
                          const sage_frontier_t* frontier, int32_t insert_self,
                          int32_t* nbr_slot, int32_t* self_slot,
                          sage_stream_t stream);

/* ---------------------------------------------------------------------------
 * sage_sample_neighbors_wide -- the same hop for the fanouts the entry above
 * refuses: aggregators.py:42-48 takes ANY num_sample, this entry any k in
 * [1, SAGE_MAX_FANOUT_WIDE].  Arguments, outputs and the draw are those of
 * sage_sample_neighbors (one wave per node, lane l owns slots l, l+64, ...;
 * draw i is word i&3 of Philox block i>>2, Floyd's walk over i = 0..k-1), so
 * for k <= SAGE_MAX_FANOUT the two entries write identical nbr / cnt, and the
 * sets stay a pure function of (seed, tag, v).  Ids outside [0, num_nodes)
 * are empty rows; rows at or past min(*n_dev, n) are not written.  With a
 * frontier: capacity >= 2 * n * (k + insert_self), rows start at the value
 * *count had, the order of nodes[] is arbitrary.
 * sage_frontier_insert and sage_forward2 keep the SAGE_MAX_FANOUT limit.
 * ------------------------------------------------------------------------- */
#define SAGE_MAX_FANOUT_WIDE 1024
int sage_sample_neighbors_wide(const int64_t* rowptr, const int32_t* col, int64_t num_nodes,
                               const int32_t* nodes, int32_t n, const int32_t* n_dev,
                               int32_t k, uint64_t seed, uint32_t tag,
                               int32_t* nbr, int32_t* cnt, int32_t* any_nonempty,
                               const sage_frontier_t* frontier, int32_t insert_self,
                               int32_t* nbr_slot, int32_t* self_slot,
                               sage_stream_t stream);

/* Insert already-sampled ids (e.g. sets injected by a caller, the reference's
 * num_sample=None path) into a frontier.  Same outputs as above. */
int sage_frontier_insert(const int32_t* nbr, const int32_t* cnt, int32_t k,
                         const int32_t* self_nodes /* nullable */,
                         int32_t n, const int32_t* n_dev,
                         const sage_frontier_t* frontier,
                         int32_t* nbr_slot, int32_t* self_slot, sage_stream_t stream);

/* ---------------------------------------------------------------------------
 * sage_gather_mean -- aggregators.py:54-74: mask build, row normalise, feature
 * fetch and mask.mm(embed_matrix), without the dense mask:
 *     out[r, :] = (1/c) * sum_{j<cnt[r]} table[row(nbr[r*k+j]), :]
 * row(x) = x, or slot_rows[x] when `slot_rows` is given (nbr then holds hash
 * slots).  self_row (nullable): aggregators.py:50-51 intended semantics -- the
 * node's own row joins the mean unless it is already among the sampled ones.
 * cnt[r]==0 (and no self row): NaN row if *any_nonempty != 0 (the reference's
 * 0/0 inside a mixed batch), else zeros (its all-empty batch); with
 * any_nonempty == NULL the row is zeros.
 * ------------------------------------------------------------------------- */
int sage_gather_mean(const float* table, int64_t table_rows, int64_t ld, int32_t dim,
                     const int32_t* nbr, const int32_t* cnt, int32_t k,
                     int32_t n, const int32_t* n_dev,
                     const int32_t* slot_rows, const int32_t* self_row,
                     const int32_t* any_nonempty,
                     float* out, int64_t ldo, sage_stream_t stream);

/* ---------------------------------------------------------------------------
 * sage_csr_mean (ABI 7) -- aggregators.py:47-48 with num_sample=None (every
 * neighbour, no sampling), then aggregators.py:52-74, straight from the CSR:
 *     out[r, :] = mean of table[u, :] over u in col[rowptr[v] .. rowptr[v+1]),
 *     v = nodes ? nodes[r] : r
 * self_loop: v's own row joins the mean unless v is already in its row (the
 * set-union rule of sage_gather_mean's self_row; rows need not be sorted).
 * An empty row without a self term is NaN if *any_nonempty != 0, else zeros
 * (zeros when any_nonempty is NULL).  Any dim >= 1, ld >= dim, ldo >= dim.
 * max_edges bounds the edges of the selected rows (rowptr[num_nodes] does for
 * distinct rows); it sizes the workspace.  A bound that is too small still
 * gives the right result, more slowly.  Node ids outside [0, num_nodes) are
 * empty rows; neighbour ids are clamped into the table.
 * Load balance: rows longer than SAGE_CSR_MEAN_CHUNK edges are cut into chunks
 * of that many, summed by separate waves and added in chunk order.  No float
 * atomics: a row's bits depend only on its CSR entries, the table, self_loop
 * and the flag, so csr_mean(nodes = S) == csr_mean(all)[S] bit for bit.
 * ------------------------------------------------------------------------- */
#define SAGE_CSR_MEAN_CHUNK 512
size_t sage_csr_mean_workspace_bytes(int32_t n, int64_t max_edges, int32_t dim);
int sage_csr_mean(const int64_t* rowptr, const int32_t* col, int64_t num_nodes,
                  const int32_t* nodes /* nullable: row r is node r */, int32_t n, int64_t max_edges,
                  const float* table, int64_t table_rows, int64_t ld, int32_t dim,
                  int32_t self_loop, const int32_t* any_nonempty /* nullable */,
                  float* out, int64_t ldo, void* workspace, size_t workspace_bytes, sage_stream_t stream);

/* ---------------------------------------------------------------------------
 * sage_csr_mean_indexed (additive, ABI 9) -- sage_csr_mean with the lookup of
 * aggregators.py:68-71 (embed_matrix = self.embed(indices), the 1hot /
 * node_degree initializers of aggregators.py:30-31) inside the mean: the table
 * is virtual,
 *     T[v, :] = embed[clamp(index[clamp(v)]), :],   v a node id,
 * index int32 [num_nodes], embed [embed_rows, dim] with leading dimension ld,
 * and the result is sage_csr_mean(table = T, table_rows = num_nodes) BIT FOR
 * BIT, without T ever being stored: the same chunks of SAGE_CSR_MEAN_CHUNK
 * edges, the same launches, the same fall-back for a small max_edges, the same
 * order of additions, the same any_nonempty rule.  Only the address of a row
 * changes.  The set-union self term ("row v holds v") is decided on NODE ids,
 * never on index values; the self row is embed[index[v]].
 * Node ids are clamped into [0, num_nodes) before index[] is read and index
 * values into [0, embed_rows) before embed[] is read: no read leaves either.
 * Every other argument, the workspace (sage_csr_mean_workspace_bytes) and the
 * order of validation are sage_csr_mean's; embed_rows in [1, 2^31).
 * ------------------------------------------------------------------------- */
int sage_csr_mean_indexed(const int64_t* rowptr, const int32_t* col, int64_t num_nodes,
                          const int32_t* nodes /* nullable: row r is node r */, int32_t n, int64_t max_edges,
                          const int32_t* index /* [num_nodes] */, const float* embed, int64_t embed_rows,
                          int64_t ld, int32_t dim,
                          int32_t self_loop, const int32_t* any_nonempty /* nullable */,
                          float* out, int64_t ldo, void* workspace, size_t workspace_bytes, sage_stream_t stream);

/* ---------------------------------------------------------------------------
 * sage_csr_mean_bf16 (additive, ABI 9) -- sage_csr_mean (aggregators.py:47-48
 * with num_sample=None, then aggregators.py:52-74) over a frozen feature
 * table STORED as bf16: table holds the raw 16 bits of each value, ld counts
 * elements.  bf16 is a storage format and nothing else: the caller rounds
 * once (round to nearest even), the kernel widens every element exactly
 * (bits << 16) and accumulates in fp32 in sage_csr_mean's order, so with
 * T32[i, j] = the fp32 value of table[i, j] the result is
 *     sage_csr_mean(table = T32) BIT FOR BIT, NaN results included (where
 *     two NaNs of DIFFERENT payloads meet in one addition, which payload the
 *     NaN result carries is defined by neither entry):
 * the same chunks of SAGE_CSR_MEAN_CHUNK entries, the same launches, the same
 * fall-back for a small max_edges, the same self term and any_nonempty rule.
 * Partials and out are fp32; the workspace is sage_csr_mean_workspace_bytes.
 * A lane's four columns are one 8-byte load when dim, ld and ldo are
 * multiples of 4, table is 8-byte and out 16-byte aligned; otherwise one
 * 2-byte load per column.  Every clamp, every other argument and the order of
 * validation are sage_csr_mean's, under the name csr_mean_bf16.  There is no
 * indexed form: the embedding sage_csr_mean_indexed reads is trained and
 * stays fp32.
 * ------------------------------------------------------------------------- */
int sage_csr_mean_bf16(const int64_t* rowptr, const int32_t* col, int64_t num_nodes,
                       const int32_t* nodes /* nullable: row r is node r */, int32_t n, int64_t max_edges,
                       const uint16_t* table /* bf16 bits */, int64_t table_rows, int64_t ld, int32_t dim,
                       int32_t self_loop, const int32_t* any_nonempty /* nullable */,
                       float* out, int64_t ldo, void* workspace, size_t workspace_bytes, sage_stream_t stream);

/* ---------------------------------------------------------------------------
 * sage_csr_frontier (additive, ABI 9) -- the frontier of a FULL-neighbourhood
 * hop: aggregators.py:47-53 with num_sample=None, `samp_neighs = to_neighs`
 * (+ the node itself), `unique_nodes_list = list(set.union(*samp_neighs))` and
 * the `unique_nodes` dict, straight from the CSR.  The hash frontier above
 * takes padded [n, k] lists with k <= SAGE_MAX_FANOUT; a whole row has no such
 * bound, so the id -> row map here is a plain array:
 *   pos    int32 [num_nodes], -1 = "not in the set"; holds -1 everywhere on
 *          entry (ids that already hold a row keep it and are not added again)
 *   count  int32 [1] on the device; on entry the first free row
 * On return nodes_out[0 .. *count) holds every distinct id among seeds[0..n)
 * and col[rowptr[v] .. rowptr[v+1]) for each seed v, each once, in ARBITRARY
 * order (as sage_frontier_t's nodes[]), pos[nodes_out[i]] == i, and pos is
 * unchanged elsewhere: pos is the `index` sage_csr_mean_indexed reads the
 * compact rows of the next layer through.  Seeds may repeat.
 * Seed ids outside [0, num_nodes) are empty rows and are not inserted;
 * neighbour ids outside it are skipped; row pointers are clamped as
 * sage_csr_mean clamps them.  Nothing is written outside pos[0..num_nodes) and
 * nodes_out[0..max_nodes): a row index >= max_nodes is not stored in
 * nodes_out, but *count keeps counting, so *count > max_nodes tells the caller
 * of the overflow (pos then names rows that nodes_out does not hold: refill it).
 * Load balance is sage_csr_mean's: a seed row longer than SAGE_CSR_MEAN_CHUNK
 * entries is cut into chunks walked by separate waves; max_edges bounds the
 * edges of the seeds' rows and sizes the workspace exactly as there, and a
 * bound that is too small gives the same set, more slowly.  One integer
 * compare-and-swap per id decides who adds it, one integer add per wave
 * reserves the rows; no float atomics, no host synchronisation.
 * Validation, before any launch: num_nodes in [0, 2^31), n >= 0,
 * max_nodes >= 0, max_edges >= 0, then NULL arrays (SAGE_EINVAL), then the
 * workspace (short or missing: SAGE_ENOSPACE; 256-byte aligned).  n == 0
 * returns SAGE_OK without a launch.  The size query is host arithmetic (0 =
 * shape out of range).
 * sage_csr_frontier_clear: pos[nodes_out[i]] = -1 for i < min(*count,
 * max_nodes), so a persistent map is reused without an O(num_nodes) fill.
 * *count is left as it is.  Rows below the first free row of the insert are
 * the caller's: they must hold node ids or negative values (skipped).
 * ------------------------------------------------------------------------- */
size_t sage_csr_frontier_workspace_bytes(int32_t n, int64_t max_edges);
int sage_csr_frontier(const int64_t* rowptr, const int32_t* col, int64_t num_nodes,
                      const int32_t* seeds, int32_t n, int64_t max_edges,
                      int32_t* pos, int32_t* nodes_out, int32_t max_nodes, int32_t* count,
                      void* workspace, size_t workspace_bytes, sage_stream_t stream);
int sage_csr_frontier_clear(int32_t* pos, const int32_t* nodes_out, const int32_t* count,
                            int32_t max_nodes, sage_stream_t stream);

/* ---------------------------------------------------------------------------
 * sage_csr_mean_backward (additive, ABI 9) -- the adjoint of
 * sage_csr_mean(nodes = NULL, n = num_nodes) with respect to `table`.  With the
 * forward's own definitions
 *     extra_v = self_loop && v is not an entry of its own row   (set union)
 *     c_v     = deg(v) + extra_v         (entries counted with multiplicity)
 *     w_v     = c_v > 0 ? 1.0f / (float)c_v : 0         (the forward's float)
 * it stores
 *     grad_table[r, :] = sum over the entries e of row u of the TRANSPOSED CSR,
 *                        in stored order, of w_x * grad_out[x, :], x = col_t[e]
 *                        + extra_u * w_u * grad_out[u, :]          (added last)
 *     u = nodes ? nodes[r] : r
 * grad_out is [num_nodes, dim], indexed by node id, leading dimension ldg.
 * grad_table is [n, dim], leading dimension ldgt; it is STORED, not
 * accumulated: the caller zeroes nothing, a row with no terms is exact zeros.
 * Not written: columns [dim, ldgt) and rows at or past n.  Not read: rows of
 * grad_out that belong to no term (empty forward rows without a self term;
 * they may hold NaN).
 * The caller supplies the transpose (rowptr_t, col_t), built once per graph:
 * for every entry (v -> u) of the forward CSR row u of the transpose holds one
 * entry v.  The order inside a row only fixes the bits.  A wrong transpose
 * gives wrong numbers, never an access out of range: ids from col_t and nodes
 * and all row pointers are clamped as in the forward.  rowptr / col (the
 * forward's CSR) give c_v and extra_v.
 * max_edges bounds the entries of the selected transposed rows and sizes the
 * workspace; a bound that is too small costs speed only.  Every term is one
 * fma; rows longer than SAGE_CSR_MEAN_CHUNK entries are cut into chunks summed
 * by separate waves and added in chunk order.  No float atomics: a row's bits
 * depend only on its transposed entries, the weights, grad_out and self_loop,
 * so backward(nodes = S) == backward()[S] bit for bit.
 * Any dim >= 1, ldg >= dim, ldgt >= dim; 16-byte accesses when dim, ldg, ldgt
 * are multiples of 4 and both arrays are 16-byte aligned.  n == 0 returns
 * SAGE_OK without a launch.  Workspace 256-byte aligned; the query returns 0
 * for a shape out of range.
 * ------------------------------------------------------------------------- */
size_t sage_csr_mean_backward_workspace_bytes(int64_t num_nodes, int32_t n, int64_t max_edges, int32_t dim);
int sage_csr_mean_backward(const int64_t* rowptr, const int32_t* col,
                           const int64_t* rowptr_t, const int32_t* col_t, int64_t num_nodes,
                           const int32_t* nodes /* nullable: row r is node r */, int32_t n, int64_t max_edges,
                           const float* grad_out, int64_t ldg, int32_t dim, int32_t self_loop,
                           float* grad_table, int64_t ldgt,
                           void* workspace, size_t workspace_bytes, sage_stream_t stream);

/* ---------------------------------------------------------------------------
 * sage_csr_mean_backward_grouped (additive, ABI 9) -- the adjoint of
 * sage_csr_mean_indexed(nodes = NULL, n = num_nodes) with respect to `embed`:
 * what autograd does behind aggregators.py:68-74 (the scatter of mask.mm's
 * gradient through self.embed(indices)), for the whole graph and with no
 * [num_nodes, dim] intermediate.  With w_v, extra_v of sage_csr_mean_backward,
 * embedding row k receives ONE flat sequence of terms: for every node u with
 * index[u] == k, in ascending u, the entries x of row u of the transposed CSR
 * in stored order, each as fma(w_x, grad_out[x, :], acc), then u itself if
 * extra_u.  The caller supplies that sequence as a RECTANGULAR CSR
 * (rowptr_gt [num_groups + 1], col_gt: node ids, self entries included), built
 * once per graph for one self_loop; self_loop here only enters the weights
 * and must be the flag the list was built with.
 *     grad_embed[k, :] = sum over e in [rowptr_gt[k], rowptr_gt[k+1]), e
 *                        ascending, of w_x * grad_out[x, :], x = col_gt[e]
 * The arithmetic is sage_csr_mean_backward's over these longer rows: every term
 * one fma; rows longer than SAGE_CSR_MEAN_CHUNK terms are cut into chunks whose
 * partials are stored and added in chunk order, shorter ones summed in place.
 * grad_embed [num_groups, dim], leading dimension ldge, is STORED: an empty row
 * is exact zeros; columns [dim, ldge) and rows at or past num_groups are not
 * written.  No float atomics.  With index[v] = v and self_loop = 0 the result
 * equals sage_csr_mean_backward's bit for bit.
 * A wrong list gives wrong numbers, never an access out of range: ids from
 * col_gt are clamped into [0, num_nodes), row pointers into
 * [0, rowptr_gt[num_groups]] and made non-decreasing (col_gt holds at least
 * rowptr_gt[num_groups] entries).  max_edges bounds rowptr_gt[num_groups] and
 * sizes the workspace; a bound that is too small costs speed only.
 * num_groups in [0, 2^31), num_nodes >= 1 unless num_groups == 0, which
 * returns SAGE_OK without a launch.  Workspace 256-byte aligned; the query
 * returns 0 for a shape out of range.
 * ------------------------------------------------------------------------- */
size_t sage_csr_mean_backward_grouped_workspace_bytes(int64_t num_nodes, int64_t num_groups, int64_t max_edges, int32_t dim);
int sage_csr_mean_backward_grouped(const int64_t* rowptr, const int32_t* col,
                                   const int64_t* rowptr_gt, const int32_t* col_gt,
                                   int64_t num_nodes, int64_t num_groups, int64_t max_edges,
                                   const float* grad_out, int64_t ldg, int32_t dim, int32_t self_loop,
                                   float* grad_embed, int64_t ldge,
                                   void* workspace, size_t workspace_bytes, sage_stream_t stream);

/* ---------------------------------------------------------------------------
 * sage_csr_mean_backward_rows (additive, ABI 9) -- the adjoint, with respect
 * to `table` ([num_rows, dim]), of sage_csr_mean_indexed(nodes, n, index), or
 * of sage_csr_mean(nodes, n) when index is NULL: the backward of a SEED BATCH
 * embedded from its full neighbourhoods (aggregators.py:47-48 num_sample=None)
 * through the compact rows of sage_csr_frontier.  The transposed sub-graph it
 * sums over exists for this batch only and is built inside the call.
 * With the forward's own definitions, for seed row r, v = nodes[r]:
 *     extra_r = self_loop && v is not an entry of its own row   (set union)
 *     c_r     = deg(v) + extra_r         (entries counted with multiplicity)
 *     w_r     = c_r > 0 ? 1.0f / (float)c_r : 0         (the forward's float)
 * the TERMS of the batch are, in this order: for r = 0 .. n-1 the entries of
 * row v in stored order, then v itself if extra_r.  A term with node id `id`
 * goes to table row
 *     key = clamp(index ? index[clamp(id, 0, num_nodes-1)] : id, 0, num_rows-1)
 * -- exactly the forward's clamps, so the result is the adjoint of what the
 * forward computed even for a bad map, and no read or write leaves an array.
 *     grad_table[f, :] = the terms with key == f in the order above (ascending
 *                        r, then position inside the row), each as ONE
 *                        fma(w_r, grad_out[r, :], acc); more than
 *                        SAGE_CSR_MEAN_CHUNK terms: chunks summed separately,
 *                        partials added in chunk order
 * which is sage_csr_mean_backward_grouped's arithmetic over the sorted term
 * list (the terms are laid out by position, sorted by key with a stable radix
 * sort, and summed by that entry's kernels).
 * grad_out is [n, dim], indexed by seed ROW (not by node id), leading dimension
 * ldg; nodes may repeat, each row is a term source of its own; a node id
 * outside [0, num_nodes) is an empty row without a self term.  grad_table,
 * leading dimension ldgt, is STORED, not accumulated: a row with no term is
 * exact zeros; columns [dim, ldgt) are not written.  No float atomics: a row's
 * bits depend only on its own term sequence -- not on where the frontier put
 * the row, not on the other rows, not on the run.
 * max_edges bounds the entries of the selected rows.  The terms get
 * max_edges + (self_loop ? n : 0) positions, and HERE a bound that is too small
 * is not "slower only": terms at positions past that capacity are DROPPED
 * (nothing is written out of range).  *total_terms (int64 on the device,
 * nullable) receives the true term count, so the caller can tell.
 * max_edges + n must stay below 2^31 (the workspace serves either self_loop).
 * Any dim >= 1, ldg >= dim, ldgt >= dim; 16-byte accesses when dim, ldg, ldgt
 * are multiples of 4 and both arrays are 16-byte aligned.
 * Validation, before any launch: shapes (num_nodes in [0, 2^31), n >= 0,
 * max_edges >= 0, num_rows in [0, 2^31 - 1), num_rows == 0 only with n == 0,
 * dim and leading dimensions, self_loop 0 / 1), then NULL arrays (rowptr, col,
 * nodes, grad_out, grad_table: SAGE_EINVAL), then the workspace (short or
 * missing: SAGE_ENOSPACE; 256-byte aligned).  num_rows == 0 returns SAGE_OK
 * without a launch; n == 0 stores zeros in all num_rows rows.  The size query
 * is host arithmetic and returns 0 for a shape out of range.
 * ------------------------------------------------------------------------- */
size_t sage_csr_mean_backward_rows_workspace_bytes(int32_t n, int64_t max_edges, int64_t num_rows, int32_t dim);
int sage_csr_mean_backward_rows(const int64_t* rowptr, const int32_t* col, int64_t num_nodes,
                                const int32_t* nodes, int32_t n, int64_t max_edges,
                                const int32_t* index /* nullable */, int64_t num_rows,
                                const float* grad_out, int64_t ldg, int32_t dim, int32_t self_loop,
                                float* grad_table, int64_t ldgt,
                                int64_t* total_terms /* nullable, device */,
                                void* workspace, size_t workspace_bytes, sage_stream_t stream);

/* ---------------------------------------------------------------------------
 * sage_csr_mean_backward_touched (additive, ABI 9) --
 * sage_csr_mean_backward_rows for the TOUCHED table rows only, and the SGD
 * update of those rows in place: what exact mini-batches over a 1hot embedding
 * of millions of rows need, where a batch's neighbourhood names a few thousand.
 * It is to sage_csr_mean_backward_rows what sage_embed_grad_rows is to
 * sage_embed_grad.  The first twelve arguments are that entry's, with its
 * terms, clamps, weights w_r, term ORDER and its rule for a max_edges that is
 * too small (terms past max_edges + (self_loop ? n : 0) positions are DROPPED;
 * *total_terms receives the true count).  Let e_0 < e_1 < ... < e_{U-1} be the
 * distinct table rows that receive at least one term and s_u row e_u's sum, bit
 * for bit the row sage_csr_mean_backward_rows stores there for the same
 * arguments (one copy of that arithmetic serves both entry points).
 *   num_rows_out[0] = U on every call that launches (0 without a term), also
 *                     when U > max_rows: the caller sees a short buffer.
 *   rows_out / grad_rows (a nullable pair; rows_out is required with grad_rows):
 *                     for u < min(U, max_rows): rows_out[u] = e_u and
 *                     grad_rows[u, 0:dim] = s_u.  Not written: rows at or past
 *                     max_rows or U, columns [dim, ldr).
 *   table (nullable): table[e_u, c] = fma(-lr, s_u[c], table[e_u, c]) for EVERY
 *                     u < U, whatever max_rows is: one rounding (fmaf).  Rows
 *                     without a term are neither read nor written; columns
 *                     [dim, ldt) are not written.
 * At least one of grad_rows and table; with both, the gradient returned is the
 * one that was applied.
 * NOTHING costs time or memory in proportion to num_rows or num_nodes: no grid,
 * loop, fill or workspace array is sized by them; num_rows enters through the
 * sort's key bits and the clamp only.  After sage_csr_mean_backward_rows' term
 * layout and stable sort the run heads of the sorted keys are counted and
 * scanned into a run list (row, start; at most min(max_edges + n, num_rows)
 * runs, a host-known capacity), which takes the place of the row pointer over
 * the table in the chunk split; the row kernel strides over u < U, read on the
 * device.  No float atomics, no host synchronisation, no allocation.
 * Any dim >= 1, ldg >= dim, ldr / ldt >= dim where their array is given,
 * max_rows >= 1 with grad_rows; 16-byte accesses when dim and the leading
 * dimensions are multiples of 4 and the arrays are 16-byte aligned.
 * Validation, before any launch, in sage_csr_mean_backward_rows' order: shapes,
 * then NULL arrays (rowptr, col, nodes, grad_out, num_rows_out; neither
 * grad_rows nor table; grad_rows without rows_out: SAGE_EINVAL), then the
 * workspace (short or missing: SAGE_ENOSPACE; 256-byte aligned).  n == 0
 * returns SAGE_OK without a launch (num_rows_out and *total_terms are then left
 * as they were).  The size query is host arithmetic, returns 0 for a shape out
 * of range and one value for every num_rows >= max_edges + n.
 * ------------------------------------------------------------------------- */
size_t sage_csr_mean_backward_touched_workspace_bytes(int32_t n, int64_t max_edges, int64_t num_rows, int32_t dim);
int sage_csr_mean_backward_touched(const int64_t* rowptr, const int32_t* col, int64_t num_nodes,
                                   const int32_t* nodes, int32_t n, int64_t max_edges,
                                   const int32_t* index /* nullable */, int64_t num_rows,
                                   const float* grad_out, int64_t ldg, int32_t dim, int32_t self_loop,
                                   int32_t* num_rows_out,                         /* [1] device, required                       */
                                   int32_t* rows_out, float* grad_rows,           /* [max_rows], [max_rows, dim]: nullable pair */
                                   int64_t max_rows, int64_t ldr,
                                   float* table, int64_t ldt, float lr,           /* [num_rows, dim] updated in place; nullable */
                                   int64_t* total_terms /* nullable, device */,
                                   void* workspace, size_t workspace_bytes, sage_stream_t stream);

/* ---------------------------------------------------------------------------
 * sage_csr_sum (additive, ABI 9) -- the gradient of a shared embedding row.
 * aggregators.py:68-71 looks features up in a trainable nn.Embedding: node v
 * reads row index[v] (its own row for 1hot, its degree's row for node_degree),
 * so row k's gradient is the sum of grad_X[v] over the nodes v with
 * index[v] = k.  Over a RECTANGULAR CSR -- num_rows groups, entries that name
 * rows of a table of table_rows rows; the caller builds it once per graph --
 *     out[r, :] = sum of table[col[e], :] over e in [rowptr[r], rowptr[r+1]),
 *                 e ascending
 * No division, no self term, no NaN rule.  out is [num_rows, dim], leading
 * dimension ldo; every row is STORED, nothing is accumulated into: an empty row
 * is exact zeros.  Not written: columns [dim, ldo).
 * Load balance is sage_csr_mean's: rows longer than SAGE_CSR_MEAN_CHUNK entries
 * are cut into chunks of that many, summed by separate waves into workspace
 * partials and added in chunk order.  max_edges bounds rowptr[num_rows] and
 * sizes the workspace; a bound that is too small costs speed only, the bits
 * are the same.  No float atomics: a row's bits depend only on its entries and
 * the table.
 * A wrong grouping gives wrong numbers, never an access out of range: ids from
 * col are clamped into the table, row pointers into [0, rowptr[num_rows]] and
 * made non-decreasing (col holds at least rowptr[num_rows] entries).
 * Any dim >= 1, ld >= dim, ldo >= dim; 16-byte accesses when dim, ld, ldo are
 * multiples of 4 and both arrays are 16-byte aligned.  num_rows == 0 returns
 * SAGE_OK without a launch.  Workspace 256-byte aligned; the query returns 0
 * for a shape out of range.
 * ------------------------------------------------------------------------- */
size_t sage_csr_sum_workspace_bytes(int64_t num_rows, int64_t max_edges, int32_t dim);
int sage_csr_sum(const int64_t* rowptr, const int32_t* col, int64_t num_rows, int64_t max_edges,
                 const float* table, int64_t table_rows, int64_t ld, int32_t dim,
                 float* out, int64_t ldo,
                 void* workspace, size_t workspace_bytes, sage_stream_t stream);

/* ---------------------------------------------------------------------------
 * sage_embed_grad (additive, ABI 9) -- the gradient of a trainable embedding
 * read through the SAMPLED layer-1 sets: an engine whose inner column array is
 * translated (col1 = index[col], table = embed [embed_rows, dim]) leaves
 * EMBEDDING rows in nbr1, and the mean over a set (aggregators.py:60-74) hands
 * every member 1 / c of the set's gradient:
 *     grad_embed[e, :] = sum of grad_agg[t, :] * (1 / c_t) over the terms (p, j)
 *                        with t = row_order[p] (p itself when row_order is
 *                        NULL), t live, j < c_t = min(cnt[t], k), nbr[t, j] == e
 * Live rows are t in [0, min(*n_dev, n)) (n_dev nullable); an entry of
 * row_order outside them adds nothing.  Ids from nbr are clamped into
 * [0, embed_rows) as sage_gather_mean_backward_ws clamps them.  A row that is
 * a member of one set several times counts with its multiplicity.
 * ORDER is part of the contract.  A row's terms are taken in ascending (p, j)
 * and cut into consecutive chunks of SAGE_CSR_MEAN_CHUNK terms; each chunk is
 * summed from zero in term order, every term entering as ONE fused multiply-add
 * acc = fma(grad_agg[t, c], 1 / c_t, acc) (one rounding per term; 1 / c_t is
 * the fp32 quotient); the chunk partials are added from zero in chunk order; a
 * row of at most one chunk is its only partial.  So the bits depend on the
 * inputs as sets and on row_order only -- with row_order = sage_row_order's
 * output on the layer's node ids, not on where the frontier's rows sit -- and
 * never on the grid or the number of CUs.  No float atomics.
 * Every row in [0, embed_rows) of grad_embed is STORED, exact zeros where no
 * term points: the caller zeroes nothing.  Not written: columns [dim, ld) and
 * anything past row embed_rows.
 * Inverted index per call in the caller's workspace (expand in row_order
 * position -> stable radix sort by embedding row -> row pointer over the
 * embedding rows -> sage_csr_sum's chunk split): no host synchronisation, no
 * allocation.  Load balance is sage_csr_sum's: a row of 1e5 terms is summed by
 * 200 lane groups, not walked by one.
 * Limits: dim, ld, ldg multiples of 4 (ld, ldg >= dim), grad_agg / grad_embed
 * 16-byte aligned, workspace 256-byte aligned, k >= 1, n * k < 2^31,
 * 1 <= embed_rows < 2^31.  A bad argument returns SAGE_EINVAL with its name in
 * sage_last_error, a short or missing workspace SAGE_ENOSPACE, both before any
 * launch; n == 0 returns SAGE_OK without a launch (grad_embed is then left as
 * it was).  The workspace query is host arithmetic (0 = shape out of range).
 * ------------------------------------------------------------------------- */
size_t sage_embed_grad_workspace_bytes(int32_t n, int32_t k, int64_t embed_rows, int32_t dim);
int    sage_embed_grad(const float* grad_agg, int64_t ldg, int32_t dim,     /* [n, dim]: d loss / d layer-1 means        */
                       const int32_t* nbr, const int32_t* cnt, int32_t k,   /* the forward's nbr1 / cnt1: EMBEDDING rows */
                       int32_t n, const int32_t* n_dev,                     /* live rows = min(*n_dev, n); nullable      */
                       const int32_t* row_order,                            /* sage_row_order's output; nullable = 0..n-1 */
                       float* grad_embed, int64_t embed_rows, int64_t ld,   /* [embed_rows, dim], STORED                 */
                       void* workspace, size_t workspace_bytes, sage_stream_t stream);

/* ---------------------------------------------------------------------------
 * sage_embed_grad_rows (additive, ABI 9) -- sage_embed_grad for the TOUCHED
 * rows only, and the SGD update of those rows in place: what a 1hot embedding
 * of millions of rows needs, where a batch names a few hundred thousand.
 * The first nine arguments and embed_rows are sage_embed_grad's, with its
 * clamp, its live-row rule and its ORDER contract.  Let e_0 < e_1 < ... <
 * e_{U-1} be the distinct embedding rows that receive at least one term and
 * s_u row e_u's sum, bit for bit the row sage_embed_grad stores there (one
 * copy of that arithmetic serves both entry points).
 *   num_rows_out[0] = U on every call that launches (0 without a live term),
 *                     also when U > max_rows: the caller sees a short buffer.
 *   rows_out / grad_rows (a nullable pair; rows_out is required with grad_rows):
 *                     for u < min(U, max_rows): rows_out[u] = e_u and
 *                     grad_rows[u, 0:dim] = s_u.  Not written: rows at or past
 *                     max_rows or U, columns [dim, ldr).
 *   embed (nullable): embed[e_u, c] = fma(-lr, s_u[c], embed[e_u, c]) for EVERY
 *                     u < U, whatever max_rows is: one rounding (fmaf).  Rows
 *                     that no term names are neither read nor written; columns
 *                     [dim, lde) are not written.
 * At least one of grad_rows and embed; with both, the gradient returned is the
 * one that was applied.
 * NOTHING costs time or memory in proportion to embed_rows: no grid, loop,
 * memset or workspace array is sized by it; it enters through the sort's key
 * bits and the clamp only.  After sage_embed_grad's expand and stable sort the
 * run heads of the sorted keys are counted and scanned into a run list (row,
 * start; at most min(n * k, embed_rows) runs, a host-known capacity), which
 * takes the place of the row pointer in sage_embed_grad's chunk split; the row
 * kernel strides over u < U, read on the device.  No float atomics, no host
 * synchronisation, no allocation.
 * Limits and errors are sage_embed_grad's: dim, ldg multiples of 4, ldr / lde
 * >= dim and multiples of 4 where their array is given, max_rows >= 1 with
 * grad_rows, grad_agg / grad_rows / embed 16-byte aligned, workspace 256-byte
 * aligned.  Shapes are checked before pointers; SAGE_EINVAL with the name in
 * sage_last_error, SAGE_ENOSPACE for a short or missing workspace, both before
 * any launch; n == 0 returns SAGE_OK without a launch (num_rows_out is then
 * left as it was).  The workspace query is host arithmetic (0 = shape out of
 * range) and returns one value for every embed_rows >= n * k.
 * ------------------------------------------------------------------------- */
size_t sage_embed_grad_rows_workspace_bytes(int32_t n, int32_t k, int64_t embed_rows, int32_t dim);
int    sage_embed_grad_rows(const float* grad_agg, int64_t ldg, int32_t dim,     /* as sage_embed_grad ...                  */
                            const int32_t* nbr, const int32_t* cnt, int32_t k,
                            int32_t n, const int32_t* n_dev,
                            const int32_t* row_order,
                            int64_t embed_rows,
                            int32_t* num_rows_out,                               /* [1] device, required                    */
                            int32_t* rows_out, float* grad_rows,                 /* [max_rows], [max_rows, dim]: nullable pair */
                            int64_t max_rows, int64_t ldr,
                            float* embed, int64_t lde, float lr,                 /* [embed_rows, dim] updated in place; nullable */
                            void* workspace, size_t workspace_bytes, sage_stream_t stream);

/* ---------------------------------------------------------------------------
 * sage_linear_act --encoders.py:49-62 without materialising the concat:
 *     out[r, :] = act( W[:, 0:ds] . self(r) + W[:, ds:ds+dim] . agg[r, :] )
 * self(r) = self_tab[self_index ? self_index[r] : r, 0:dim]; ds = dim when
 * self_tab != NULL (concat encoder, gcn=False) else 0 (gcn=True).
 * W is [out_dim, ds+dim] row-major (ldw), exactly the reference Parameter.
 * out is [n, out_dim] (the module returns its transpose view, encoders.py:62).
 * fp32 MFMA (v_mfma_f32_32x32x2_f32): exact-fp32 products, fp32 accumulate.
 * ------------------------------------------------------------------------- */
int sage_linear_act(const float* self_tab, int64_t ld_self, const int32_t* self_index,
                    const float* agg, int64_t ld_agg, int32_t dim,
                    const float* weight, int64_t ldw, int32_t out_dim, int32_t act,
                    int32_t n, const int32_t* n_dev,
                    float* out, int64_t ldo, sage_stream_t stream);

/* ---------------------------------------------------------------------------
 * sage_layer_forward -- one Encoder.forward (encoders.py:47-62) in ONE launch:
 * gather-mean rows are staged through an LDS tile and contracted with W by
 * fp32 MFMA without the [n, dim] round trip through HBM.  Arguments as the two
 * calls above.  Rows at or past min(*n_dev, n) are not written, nor are the
 * columns [out_dim, ldo) of out.  Neighbour ids (after slot_rows) and the
 * concat self_index are clamped into the table.  SAGE_EUNSUPPORTED if
 * (dim, out_dim) has no fused kernel, if table or weight is not 16-byte
 * aligned, or if ld or ldw is not a multiple of 4; nothing is launched and
 * the caller then uses the two-launch form.
 * ------------------------------------------------------------------------- */
int sage_layer_forward(const float* table, int64_t table_rows, int64_t ld, int32_t dim,
                       const int32_t* nbr, const int32_t* cnt, int32_t k,
                       int32_t n, const int32_t* n_dev,
                       const int32_t* slot_rows, const int32_t* self_row,
                       const int32_t* any_nonempty,
                       int32_t concat, const int32_t* self_index,
                       const float* weight, int64_t ldw, int32_t out_dim, int32_t act,
                       float* out, int64_t ldo, sage_stream_t stream);
int sage_layer_forward_supported(int32_t dim, int32_t out_dim, int32_t concat);

/* ---------------------------------------------------------------------------
 * sage_layer1_fused (ABI 8) -- sage_gather_mean + the gcn encoder's W.x + act on a SLICE-MAJOR table of 32-float slices
 * (float[d0 / 32][table_rows][32], sage_model_t.table_sliced) in ONE launch that keeps the means on the chip: a block walks the
 * slices of its 32 rows in phases, gathers a slice as the column-sliced gather does and contracts it with that slice of the
 * prepared W (sage_prepare_weights(weight, ldw, d0, out_dim, 0, ...); required) while the fp32 accumulators stay in registers.
 *     out[r, :] = act( W . mean_j table[nbr[r*k+j], :] ),  rows r < min(*n_dev, n)
 * Same self_row / any_nonempty rules as sage_gather_mean (no slot_rows); the bits are those of sage_gather_mean on that table
 * followed by the contraction, whatever n and wherever the row sits.  d0 in {64, 128, 256}, out_dim in {32, 64, 96, 128},
 * k <= SAGE_MAX_FANOUT, ldo % 4 == 0, 16-byte aligned arrays; otherwise SAGE_EUNSUPPORTED and nothing is launched.
 * ------------------------------------------------------------------------- */
int sage_layer1_fused_supported(int32_t d0, int32_t out_dim, int32_t k);
int sage_layer1_fused(const float* table_sliced, int64_t table_rows, int32_t d0,
                      const int32_t* nbr, const int32_t* cnt, int32_t k,
                      int32_t n, const int32_t* n_dev,
                      const int32_t* self_row, const int32_t* any_nonempty,
                      const float* weight, int64_t ldw, const void* weight_prepared, int32_t out_dim, int32_t act,
                      float* out, int64_t ldo, sage_stream_t stream);

/* ---------------------------------------------------------------------------
 * Backward of the two operators (autograd of encoders.py:58-62 and
 * aggregators.py:60-74; the reference gets these from torch autograd through
 * mm / relu / cat / div).
 *
 * sage_linear_act_backward: dZ = grad_out * act'(out);
 *   grad_weight[out_dim, ds+dim] += dZ^T . [self | agg]   (ACCUMULATES: caller zeroes; nullable)
 *   grad_x[n, ds+dim]             = dZ . W                 (written; nullable)
 *   Columns [ds+dim, ldgw) of grad_weight and [ds+dim, ldgx) of grad_x are
 *   not written.
 * sage_gather_mean_backward: grad_table[row(nbr[r,j]), :] += grad_agg[r, :] / c
 *   (fp32 atomics, caller zeroes grad_table; same slot_rows / self_row rules
 *   as the forward: neighbour ids (after slot_rows) and the self row are
 *   clamped into [0, table_rows) exactly as the forward clamps them, the
 *   set-union test compares the self row before clamping, so c is the
 *   forward's and the result is the adjoint of sage_gather_mean).
 * ------------------------------------------------------------------------- */
/* n_dev (nullable): the live row count on the device, min(*n_dev, n) rows take part (rows past it are neither read nor written:
 * they add nothing to grad_weight or grad_table, and their rows of grad_x keep what the caller left there). */
int sage_linear_act_backward(const float* self_tab, int64_t ld_self, const int32_t* self_index,
                             const float* agg, int64_t ld_agg, int32_t dim,
                             const float* weight, int64_t ldw, int32_t out_dim, int32_t act,
                             const float* out, int64_t ldo, const float* grad_out, int64_t ldg,
                             int32_t n, const int32_t* n_dev,
                             float* grad_weight, int64_t ldgw, float* grad_x, int64_t ldgx,
                             sage_stream_t stream);
int sage_gather_mean_backward(const float* grad_agg, int64_t ldg, int32_t dim,
                              const int32_t* nbr, const int32_t* cnt, int32_t k,
                              int32_t n, const int32_t* n_dev,
                              const int32_t* slot_rows, const int32_t* self_row,
                              float* grad_table, int64_t table_rows, int64_t ld,
                              sage_stream_t stream);

/* Reproducible forms (ABI 3).  torch autograd on the reference's CPU (model.py:249) gives the same bits run after run; the two
 * entry points above add in order of arrival (fp32 atomics).  These take a caller-owned workspace instead and are bitwise
 * reproducible for given inputs and launch tunables:
 *  - sage_linear_act_backward_ws: the reduction over the n rows is cut into row ranges, every range STORES its partial
 *    [out_dim, ds+dim] tile in the workspace, one kernel adds the partials in range order to grad_weight (still "+=": the
 *    caller zeroes).  grad_x as above.  Even widths / leading dimensions and 8-byte aligned arrays take the fast kernel (operands
 *    straight from HBM in MFMA register order); anything else the generic tile kernel, also through partials.
 *  - sage_gather_mean_backward_ws: an inverted index (expand -> stable radix sort by table row -> run heads) built per call in
 *    the workspace; every table row's terms are then summed in ascending (r, j) order and the row is STORED (zeros where
 *    nobody points): rows [0, min(*table_rows_dev, table_rows)) of grad_table are written, the caller zeroes nothing; rows past
 *    them and columns [dim, ld) are not.  Ids are clamped as in the legacy form.  Needs dim % 4 == 0, ld % 4 == 0, 16-byte aligned
 *    arrays; otherwise, and for a short workspace, nothing is launched.
 * The *_workspace_bytes queries are host-side arithmetic (0 = shape out of range / query failed); workspaces 256-byte aligned. */
size_t sage_linear_act_backward_workspace_bytes(int32_t n, int32_t dim, int32_t has_self, int32_t out_dim);
int sage_linear_act_backward_ws(const float* self_tab, int64_t ld_self, const int32_t* self_index,
                                const float* agg, int64_t ld_agg, int32_t dim,
                                const float* weight, int64_t ldw, int32_t out_dim, int32_t act,
                                const float* out, int64_t ldo, const float* grad_out, int64_t ldg,
                                int32_t n, const int32_t* n_dev,
                                float* grad_weight, int64_t ldgw, float* grad_x, int64_t ldgx,
                                const int32_t* row_order /* nullable */,
                                void* workspace, size_t workspace_bytes, sage_stream_t stream);
/* The frontier's rows are in arbitrary order (aggregators.py:52: so is a Python set), and the weight gradient is a sum over the
 * layer's rows: for the same bits run after run it has to add them in an order that does not depend on the layout.  sage_row_order
 * writes that order -- rows [0, first_row) as they are (the concat encoder's own seeds), then the live rows [first_row, *n_dev) by
 * ascending node id (distinct there), dead rows last -- and sage_linear_act_backward_ws(row_order = it) sums its k-th term from row
 * row_order[k] (grad_weight only; grad_x is per row).  nodes: int32[n], the layer's node ids (sage_ws_layout_t.s1_nodes). */
size_t sage_row_order_workspace_bytes(int32_t n);
int sage_row_order(const int32_t* nodes, int32_t n, const int32_t* n_dev, int32_t first_row, int32_t* order,
                   void* workspace, size_t workspace_bytes, sage_stream_t stream);
/* Layer-1 weight gradient of the TWO-LAYER stack (model.py:219-222 differentiated, model.py:249), summed over the outer samples
 * instead of over the layer-1 rows: grad_w1 [h1, d0 or 2*d0] += sum over the seeds r, in order, of
 *   (concat)  act1'(h1[r]) . grad_x2[r, 0:h1]  (x)  [table[s1_nodes[r]] | agg1[r]]                    (the seed's own layer-1 row)
 *   for j < cnt2[r] (and the self-loop row):  act1'(h1[t]) . grad_x2[r, off:off+h1] / c_r  (x)  [table[s1_nodes[t]] |] agg1[t],  t = row2[r, j]
 * (off = h1 for the concat encoder, else 0; c_r as in the forward).  Mathematically the chain mean-backward -> relu' -> dZ^T.X; in
 * this form no grad_h1 is scattered and the terms come in (seed, slot) order, which does not depend on the frontier's arbitrary row
 * order: bitwise reproducible without an inverted index or a canonical row order (csrc/sage_backward.hip).  grad_x2 is what
 * sage_linear_act_backward(_ws) returned for layer 2; row2 / cnt2 / self_row2 / h1 / agg1 / s1_nodes are the forward's
 * intermediates (sage_ws_layout_t).  Widths and leading dimensions multiples of 4, arrays 16-byte aligned; otherwise, and for a
 * short workspace, nothing is launched.  Rows of h1 / agg1 / the table that no term references contribute nothing
 * (a NaN there stays out of grad_w1); columns past d0 (concat: 2*d0) of grad_w1 are not written. */
size_t sage_two_hop_grad_w1_workspace_bytes(int32_t batch, int32_t k2, int32_t d0, int32_t concat, int32_t h1);
int sage_two_hop_grad_w1(const float* grad_x2, int64_t ldgx,
                         const int32_t* row2, const int32_t* cnt2, int32_t k2, const int32_t* self_row2, int32_t batch,
                         const float* h1, int64_t ldh, int32_t h1_dim, int32_t act1,
                         const float* agg1, int64_t lda, int32_t d0,
                         int32_t concat, const float* table, int64_t table_ld, const int32_t* s1_nodes,
                         float* grad_w1, int64_t ldgw,
                         void* workspace, size_t workspace_bytes, sage_stream_t stream);
size_t sage_gather_mean_backward_workspace_bytes(int32_t n, int32_t k, int64_t table_rows);
int sage_gather_mean_backward_ws(const float* grad_agg, int64_t ldg, int32_t dim,
                                 const int32_t* nbr, const int32_t* cnt, int32_t k,
                                 int32_t n, const int32_t* n_dev,
                                 const int32_t* slot_rows, const int32_t* self_row,
                                 float* grad_table, int64_t table_rows, const int32_t* table_rows_dev, int64_t ld,
                                 void* workspace, size_t workspace_bytes, sage_stream_t stream);

/* ---------------------------------------------------------------------------
 * Two-layer forward: model.py:219-222 wiring of two Encoders, i.e. the
 * "2-hop forward" the headline metric counts.
 * ------------------------------------------------------------------------- */
/* A batch descriptor in DEVICE memory: which seeds to embed and the sampler key to use.
 * A ring of them + a device-side cursor lets a captured hipGraph of sage_forward2 be
 * replayed for batch after batch with NO per-replay host work: every kernel takes its
 * seeds pointer and key from queue[*cursor % queue_len], and the last node of the
 * forward advances the cursor. */
typedef struct {
    const int32_t* seeds;   /* [batch] device pointer */
    uint64_t       seed;    /* sampler key for this batch */
} sage_batch_t;

typedef struct {
    /* Each Encoder holds its own adjacency (encoders.py:21); model.py passes the
     * same dict to both.  Injecting pre-sampled sets (the reference's
     * num_sample=None switch, aggregators.py:47-48) = pointing a layer at a CSR
     * whose rows ARE the sampled sets, with k >= the longest row. */
    const int64_t* rowptr1;     /* [num_nodes+1]  enc1.adj_lists (inner hop)       */
    const int32_t* col1;
    const int64_t* rowptr2;     /* [num_nodes+1]  enc2.adj_lists (outer hop)       */
    const int32_t* col2;
    int64_t        num_nodes;
    const float*   table;       /* [num_nodes, d0] raw features (model.py:214-215) */
    int64_t        table_ld;
    int32_t        d0;
    const float*   w1;          /* [h1, d0 or 2*d0]   enc1.weight                  */
    int32_t        h1;
    const float*   w2;          /* [h2, h1 or 2*h1]   enc2.weight                  */
    int32_t        h2;
    int32_t        k1;          /* enc1.num_sample (inner hop)                     */
    int32_t        k2;          /* enc2.num_sample (outer hop, on the seeds)       */
    int32_t        concat;      /* 1: encoder gcn=False (self || agg); 0: gcn=True */
    int32_t        agg_self_loop;/* aggregator gcn flag (aggregators.py:50-51)     */
    int32_t        act1, act2;  /* SAGE_ACT_*                                     */
    int32_t        nan_empty;   /* 1: reference NaN rule for empty sets; 0: zeros  */
    int32_t        fused;       /* 1: one-launch layers when supported; 0: never   */
    int32_t        ws_batch;    /* batch size the workspace was laid out and initialised for (sage_forward2_init);
                                   forwards may use any batch <= ws_batch.  0 = the call's own batch.          */
    /* optional batch queue (all NULL/0 = take `seeds` and `seed` from the call arguments) */
    const sage_batch_t* queue;  /* [queue_len] descriptors in device memory            */
    int32_t        queue_len;
    int32_t*       queue_cursor;/* [1] device counter, advanced by one per forward      */
    /* optional (ABI 2): enc1.weight already split into bf16 planes by sage_prepare_weights (NULL = the kernel
     * splits its slice itself at every launch).  Must be refreshed whenever w1 changes (an optimizer step). */
    const void*    w1_prepared;
    /* optional (ABI 2): caller id -> internal id, int32[num_caller_ids].  An engine that keeps graph and table in an
     * order of its own (sage355.engine: rows sorted by descending degree, so that the most-gathered feature rows are
     * neighbours in HBM) translates every seed with it INSIDE the outer-hop kernel; NULL = ids are used as they are. */
    const int32_t* seed_map;
    /* optional (ABI 3): a second copy of the table in SLICE-MAJOR order, float[d0 / W][num_nodes][W], W = table_slice_floats (d0 % W == 0): the
     * column-sliced layer-1 gather then reads one contiguous array per 256-byte slice.  NULL = gather from `table`. */
    const float*   table_sliced;
    int32_t        table_slice_floats;  /* floats per slice of table_sliced: 64 (256-byte slices; 0 means 64) or 32 / 128; d0 % it == 0 */
    /* optional (ABI 4): the caller DECLARES that w1 is the identity matrix [h1, h1] (d0 == h1, gcn encoder) -- serving on a pre-transformed
     * table, Y = X . W1^T computed once per weight update (sage355.engine.pretransform_table): layer 1 is then act1(mean(Y[nbrs])).  When
     * layer 1 runs in its split form the contraction is skipped and the column-sliced gather applies act1 and writes h1 itself; everywhere
     * else the flag is ignored (the contraction with an identity W1 returns its operand exactly, so the result is the same bit for bit).
     * w1 must still point at a real identity matrix. */
    int32_t        w1_is_identity;
    /* (ABI 8) the caller needs the layer-1 means of this forward (sage_ws_layout_t.agg1: the backward reads them, sage_two_hop_grad_w1):
     * layer 1 then always runs as gather + contraction when it is split.  0: the library may run the split layer 1 as ONE launch that
     * never writes the means (sage_layer1_fused below; bit-identical h1), and agg1 is then left as it was. */
    int32_t        keep_means;
} sage_model_t;

/* Where the intermediates of one forward live inside the caller's workspace
 * (byte offsets).  Tests and the benchmark's parity gate read the sampled sets
 * back through this; h1 is what layer 2 consumes. */
typedef struct {
    size_t  total_bytes;
    size_t  counters;     /* int32[8]: [0] frontier rows claimed (|S1| = first row + this), [1] any_nonempty
                             outer, [2] any_nonempty inner, [7] completion ticket; all zero between forwards.
                             int32[8..15]: copy of [0..7] as the LAST forward left them (read-back only)          */
    size_t  hash_keys, hash_rows; int32_t hash_capacity;
    size_t  s1_nodes;     /* int32[max_s1]  layer-1 node ids; concat: rows [0,B) are the seeds */
    int32_t max_s1;
    size_t  nbr2, slot2, cnt2, self_slot2;   /* int32 [B,k2] [B,k2] [B] [B]  */
    size_t  row2, self_row2;                 /* int32 [B,k2] [B]: frontier ROW of every outer sample */
    size_t  nbr1, cnt1;                      /* int32 [max_s1,k1] [max_s1]   */
    size_t  agg1;         /* float [max_s1, d0]   (two-launch form only)     */
    size_t  h1;           /* float [max_s1, h1]                               */
    size_t  agg2;         /* float [B, h1]        (two-launch form only)     */
    int32_t layer1_split; /* 1: layer 1 runs as column-sliced gather -> agg1 -> dense contraction;
                             0: one fused launch (or the generic two-launch form when unsupported)   */
} sage_ws_layout_t;

int sage_forward2_layout(const sage_model_t* m, int32_t max_batch, sage_ws_layout_t* layout_host);

/* The workspace is self-cleaning: each forward wipes the hash keys it used and its last
 * kernel zeroes the device counters, so a forward is 4-5 launches with no memset / reset.
 * sage_forward2_init puts a freshly allocated workspace into that state (call it once,
 * with the LARGEST batch the workspace will see, and use one batch size per workspace
 * thereafter: the layout, hence the key array, depends on it). */
int sage_forward2_init(const sage_model_t* m, void* workspace, size_t workspace_bytes,
                       int32_t max_batch, sage_stream_t stream);

/* seeds int32[batch]; out float[batch, h2] (ldo).  Enqueues the whole forward
 * on `stream`; no host synchronisation.  The sampled sets are a pure function
 * of (seed, node id, hop tag).  With m->queue set, `seeds` and `seed` are ignored
 * (seeds may be NULL) and the call is safe to capture into a hipGraph. */
int sage_forward2(const sage_model_t* m, void* workspace, size_t workspace_bytes,
                  const int32_t* seeds, int32_t batch, uint64_t seed,
                  float* out, int64_t ldo, sage_stream_t stream);

/* Same forward with hipEvent_t markers around its stages, for in-situ kernel timing
 * (bench.py roofline).  stage_events: 2*SAGE_NUM_STAGES hipEvent_t handles
 * (begin, end for interval 0..4 = outer sample, inner sample, layer-1 gather (split layers
 * only, else empty), layer-1 contraction or fused layer 1, layer 2); NULL entries are skipped.
 * Events are recorded on `stream`. */
#define SAGE_NUM_STAGES 5
int sage_forward2_profiled(const sage_model_t* m, void* workspace, size_t workspace_bytes,
                           const int32_t* seeds, int32_t batch, uint64_t seed,
                           float* out, int64_t ldo, sage_stream_t stream,
                           void* const* stage_events);

/* ---------------------------------------------------------------------------
 * Weight preparation for the layer-1 contraction (encoders.py:58-61, `self.weight.mm(combined.t())`).
 * The contraction runs on the bf16 matrix pipe with fp32 accuracy: x.w = sum over the products of the three
 * bf16 terms of x and of w (csrc/sage_dense.hip).  Splitting W [out_dim, dim] into its three bf16 planes,
 * laid out in the kernel's register order, depends only on W, so it can be done once per weight update instead
 * of by every block of every launch (a third of the contraction's time at BASELINE config 3).
 * With concat != 0, W is [out_dim, 2 * dim] in the [self | agg] order of encoders.py:54.
 * sage_prepared_weight_bytes: size of the prepared form (planes + a 16-byte trailer that marks a W holding
 * |w| >= 2^127 / Inf / NaN), 0 if the shape is not one of the contraction kernel's (out_dim > 128, dim % 4 != 0).
 * Results are bit-identical with and without the prepared form.
 * ------------------------------------------------------------------------- */
size_t sage_prepared_weight_bytes(int32_t dim, int32_t out_dim, int32_t concat);
int sage_prepare_weights(const float* weight, int64_t ldw, int32_t dim, int32_t out_dim, int32_t concat,
                         void* prepared, size_t prepared_bytes, sage_stream_t stream);

/* ---------------------------------------------------------------------------
 * Role pipeline: consecutive forwards software-pipelined over ROLE STREAMS (csrc/sage_pipe.hip).
 * Each stage of the forward -- S: outer + inner sample, G: layer-1 gather, D: layer-1 contraction,
 * L: layer 2 -- is enqueued on a HIP stream of its own and consecutive batches move through the
 * stages over `depth` workspaces; hipEvents carry S(b) -> G(b) -> D(b) -> L(b) -> S(b + depth).
 * In steady state one stage (the gather) is on the critical path instead of the sum of five.
 * Results are bit-identical to sage_forward2 on the same (seeds, key).  The pipe owns only its
 * hipEvents; workspaces (each laid out by sage_forward2_layout and initialised by
 * sage_forward2_init for m->ws_batch / `batch`), streams and outputs belong to the caller.
 * streams[4] = {S, G, D, L}; entries may coincide (the event between two roles on one stream is
 * skipped).  All calls are host-side enqueues (eleven stream operations per batch); sage_pipe_fork / sage_pipe_join
 * order the pipe against the caller's own stream.  The whole pattern -- hipStreamBeginCapture(stream), sage_pipe_fork(stream),
 * submits (the first `depth` of them on free workspaces: segment_start, or sage_pipe_reset before), sage_pipe_join(stream),
 * hipStreamEndCapture -- can be captured into ONE hipGraph (ABI 3): while the role streams are capturing, the workspace-release
 * edge L(b) -> S(b + depth) is added as an explicit node dependency, because waiting for it by event crashes
 * hipStreamEndCapture on ROCm 7.2 (csrc/sage_pipe.hip, experiments/r03/capture_repro.cpp).  The captured graph embeds the seeds
 * pointers and keys of the batches it was captured with.  After a capture, call sage_pipe_reset before eager submission.
 * Host enqueue threads (ABI 4): sage_pipe_set_threads(p, 1, window) starts one host thread per role; a submit then only POSTS the
 * batch and each role's thread makes that role's HIP calls on its stream (thirteen HIP calls per batch are 40-60 us on one host
 * thread -- as long as the GPU's period), ordered across threads as hipEvent semantics need.  sage_pipe_flush returns when every
 * posted batch has been enqueued (and reports a role thread's error); join / fork / reset / update_weights / destroy flush first.
 * A caller that synchronises the DEVICE or the role streams itself must flush first.  Needs four distinct role streams.
 * Not thread safe per pipe (one submitting thread).
 * Replaces nothing in the reference (model.py:240-252 runs one batch at a time).
 * ------------------------------------------------------------------------- */
#define SAGE_PIPE_MAX_DEPTH 8
typedef struct sage_pipe sage_pipe_t;
int sage_pipe_create(const sage_model_t* m, int32_t batch, int32_t depth, void* const* workspaces,
                     size_t workspace_bytes, const sage_stream_t* streams, sage_pipe_t** out);
int sage_pipe_destroy(sage_pipe_t* p);
/* The pipe keeps a COPY of *m; after an optimizer step (new pointers and / or freshly prepared planes; the caller
 * orders the role streams behind whatever wrote them, e.g. with sage_pipe_fork): */
int sage_pipe_update_weights(sage_pipe_t* p, const float* w1, const float* w2, const void* w1_prepared);
/* One batch: seeds int32[batch] and out float[batch, h2] must stay valid until the batch has left stream L. */
int sage_pipe_submit(sage_pipe_t* p, const int32_t* seeds, uint64_t key, float* out, int64_t ldo);
/* sage_pipe_submit + two caller-owned hipEvent_t (gather_events[0], [1]) that the layer-1 gather launch carries as its own
 * start / stop events on whichever stream it takes (stream G, or stream D for an odd batch of the alternating placement below; column-sliced
 * and phase-sliced layer 1; left unrecorded where the gather stage launches nothing). */
int sage_pipe_submit_profiled(sage_pipe_t* p, const int32_t* seeds, uint64_t key, float* out, int64_t ldo,
                              void* const* gather_events);
/* n batches from one host loop: batch i reads seeds + i*seed_stride (elements), keys_host[i] (HOST array) and
 * writes out + (i % out_slots)*out_stride.  segment_start != 0: the first `depth` batches of this call find
 * their workspaces free (the caller has joined everything submitted before). */
int sage_pipe_submit_many(sage_pipe_t* p, const int32_t* seeds, int64_t seed_stride, const uint64_t* keys_host,
                          int32_t n, float* out, int64_t ldo, int64_t out_stride, int32_t out_slots,
                          int32_t segment_start);
/* `stream` waits for everything submitted so far / every role stream waits for `stream`. */
int sage_pipe_join(sage_pipe_t* p, sage_stream_t stream);
int sage_pipe_fork(sage_pipe_t* p, sage_stream_t stream);
/* Forget every submit (the next `depth` submits find their workspaces free); the caller has joined / synchronised all of them. */
int sage_pipe_reset(sage_pipe_t* p);
/* on != 0: start the four host enqueue threads (on == 0: drain and stop them).  window > 0: role S enqueues batch b only once batch
 * b - window has left the GPU, which bounds how far the host runs ahead (0 = unbounded; window < 32). */
int sage_pipe_set_threads(sage_pipe_t* p, int32_t on, int32_t window);
/* Every posted batch has been enqueued on the role streams (not: has run).  Returns the first error a role thread met. */
int sage_pipe_flush(sage_pipe_t* p);
/* Express lane (ABI 6).  A batch submitted to an IDLE pipe -- every earlier batch has left layer 2, found with one hipEventQuery -- is
 * enqueued whole on stream L, like sage_forward2, instead of being handed from stream to stream: four record + wait pairs of ~11 us
 * each on an otherwise empty GPU (141 -> ~90 us to the first output of a region; the batches behind it start on the role streams at
 * once).  Same kernels and workspace, bit-identical results; never inside a stream capture; needs four distinct role streams;
 * SAGE_PIPE_EXPRESS=0 (environment, read once) turns it off.  Returns how many batches of this pipe took it so far (-1: NULL pipe). */
int64_t sage_pipe_express_count(const sage_pipe_t* p);
/* Alternating layer-1 streams (additive, ABI 9).  While stage D launches nothing (the one-launch layer 1, the gather-only form), role
 * G's calls for every odd batch -- counted from the last reset -- go to stream D's idle queue instead of stream G's: consecutive
 * layer-1 launches are then ordered by their data alone and the ~10 us between two launches of one queue close.  Same kernels, events,
 * workspaces and arguments, bit-identical results; never inside a stream capture or for an express batch; needs four distinct role
 * streams.  Taken when stream L was created with a HIGHER priority than streams G and D (hipStreamCreateWithPriority; layer 2 must be
 * able to claim the CUs a retiring layer-1 launch frees before the next launch's blocks do: with equal priorities the placement is
 * 4-5 us per forward slower, not faster); SAGE_PIPE_G_ALT=0 / 1 (environment, read once) forces it off / on.
 * Returns how many batches of this pipe had their layer 1 on stream D so far (-1: NULL pipe). */
int64_t sage_pipe_alternate_count(const sage_pipe_t* p);
/* Inner sampler in front of layer 1 (additive, ABI 9).  Wherever the pipe alternates its layer-1 streams (above), role S launches only
 * the outer hop of a batch and role G launches the inner hop and then layer 1, one behind the other on the batch's layer-1 stream (G
 * for even, D for odd batches): stream S is no longer a serial chain of two samplers per batch, and the stream-to-stream hand-off sits
 * between the two hops instead of in front of a layer 1 that waits for nothing else.  Layer 2 of such a batch runs in 512-thread
 * blocks (the 1024-thread form starves beside two layer-1 launches and a sampler).  Same kernels, events, workspaces and
 * arguments, bit-identical results; never inside a stream capture, for an express batch, without the alternation, or with the fused
 * sampler (SAGE_SAMPLE_FUSED=1: one launch for both hops).  SAGE_PIPE_SI_WITH_L1=0 / 1 (environment, read once) forces it off / on
 * where the alternation is taken; unset, the pipe takes it.
 * Returns how many batches of this pipe had their inner sampler launched in front of their layer 1 so far (-1: NULL pipe). */
int64_t sage_pipe_inner_with_layer1_count(const sage_pipe_t* p);

/* ---------------------------------------------------------------------------
 * Classifier head (ABI 9): SupervisedGraphSage's scores, CrossEntropyLoss and the three gradients that follow
 * (model.py:59-69: `scores = self.weight.mm(embeds)`, `self.xent(scores.t(), labels)`; model.py:249: `loss.backward()`)
 * as one row-tiled kernel plus one fixed-order reduce.  Per row r of emb [n, dim], with w_cls [C, dim] the reference's Parameter:
 *   s[r, c] = sum_d emb[r, d] * w_cls[c, d]        m_r = max_c s[r, c]        lse_r = m_r + log sum_c exp(s[r, c] - m_r)
 *   loss           = scale * sum_r (lse_r - s[r, labels[r]])        (scale = 1 / n, or 1 / global_batch for a data-parallel shard)
 *   g[r, c]        = scale * (softmax(s[r, :])[c] - [c == labels[r]])
 *   grad_emb[r, :] = sum_c g[r, c] * w_cls[c, :]
 *   grad_w[c, :]   = sum_r g[r, c] * emb[r, :]      STORED, not accumulated: the caller zeroes nothing, and what grad_w and the
 *                                                   workspace held before the call does not matter
 *   pred[r]        = first index of the maximum of s[r, :]; a NaN counts as the maximum (torch.argmax)
 * A row whose label lies outside [0, C) adds nothing to the loss and has g[r, :] = 0; the label is never used as an index; its
 * scores and pred are still written.  labels == NULL is the inference form: loss, grad_emb and grad_w must be NULL too and only
 * scores / pred are produced.  Every output is nullable.  NaN and Inf propagate as the arithmetic dictates, nothing is clamped.
 * Columns [dim, ldg) of grad_emb, [dim, ldgw) of grad_w and [C, lds) of scores are not written; columns [dim, lde) of emb are not read.
 * Order of the sums: no float atomics, every sum runs in an order fixed by (n, C, dim) alone.  The rows are cut into ranges of
 * SAGE_HEAD_RANGE_ROWS; each range STORES its partial [C, dim] tile of grad_w and its partial loss in the workspace, terms in
 * ascending row order; a second kernel adds the partials in range order and stores grad_w and loss.  scores, pred and grad_emb of
 * a row depend on that row, w_cls, its label and scale only: row r of a call with n rows has the bits of row r of a call with
 * more rows.  Everything is fp32, the dots are plain FMA chains in ascending d / c / r.
 * Host validation, before any launch: NULL emb / w_cls / workspace, n < 1, a leading dimension shorter than its width, loss or
 * gradients requested without labels: SAGE_EINVAL; dim outside [4, SAGE_HEAD_MAX_DIM] or dim % 4 != 0, num_classes outside
 * [1, SAGE_HEAD_MAX_CLASSES], lde / ldw / ldg / ldgw not a multiple of 4, emb / w_cls / grad_emb / grad_w / workspace not 16-byte
 * aligned: SAGE_EUNSUPPORTED; short workspace: SAGE_ENOSPACE.  sage_xent_head_supported and sage_xent_head_workspace_bytes are
 * host arithmetic (the latter 0 for an unsupported shape or n < 1).
 * ------------------------------------------------------------------------- */
#define SAGE_HEAD_MAX_CLASSES 64
#define SAGE_HEAD_MAX_DIM     256
#define SAGE_HEAD_RANGE_ROWS  64      /* rows per partial: a constant, NOT a tunable (it fixes the order of the sums) */
int    sage_xent_head_supported(int32_t dim, int32_t num_classes);
size_t sage_xent_head_workspace_bytes(int32_t n, int32_t dim, int32_t num_classes);
int    sage_xent_head(const float* emb, int64_t lde, int32_t dim,            /* [n, dim]                      */
                      const float* w_cls, int64_t ldw, int32_t num_classes,   /* [C, dim], the reference Parameter */
                      const int64_t* labels /* [n], nullable */, int32_t n, float scale,
                      float* scores   /* [n, C]   nullable */, int64_t lds,
                      int32_t* pred   /* [n]      nullable */,
                      float* loss     /* [1]      nullable */,
                      float* grad_emb /* [n, dim] nullable */, int64_t ldg,
                      float* grad_w   /* [C, dim] nullable, STORED */, int64_t ldgw,
                      void* workspace, size_t workspace_bytes, sage_stream_t stream);

/* ---------------------------------------------------------------------------
 * sage_pagerank_* (additive, ABI 9) -- the `pagerank` initializer.
 * model.py:158-162 (and its copies at 322-326 and 470-474) calls nx.pagerank(G)
 * with its defaults and uses the result as the single feature column, layer 1
 * through a sigmoid (encoders.py:58).  These entries are that power iteration on
 * the device, one step per call, as a PULL over a CSR whose row i lists the
 * nodes that link to i -- for a symmetric graph its own CSR, for out-edge lists
 * their transpose with out_degree taken from the original rows:
 *     s_i      = sum of y[col[e]] over e in [rowptr[i], rowptr[i+1])
 *     x_next_i = alpha * (s_i + mass / N) + (1 - alpha) / N
 *     y_next_i = x_next_i * inv_out[i]
 *     err      = sum over i of |x_next_i - x_i|
 * with y = x * inv_out, inv_out[j] = 1 / out-degree of j (0 for a dangling
 * node) and mass = the sum of x_j over the dangling nodes: uniform start 1 / N,
 * uniform personalization and dangling weights, every stored entry (a self loop
 * too) one link of weight 1.  The caller stops after the first step whose
 * err < N * tol (nx: tol = 1e-6, max_iter = 100, alpha = 0.85).
 * state is float[2] on the device: {err of the last step, mass of the current
 * x}; a step reads state[1] and stores both.  All arrays are fp32 [N] except
 * rowptr (int64 [N + 1]), col (int32, at least rowptr[N] entries) and
 * out_degree (int32 [N]).
 * Order of the sums (csrc/sage_pagerank.hip states it in full): the bits of
 * x_next[i] depend on row i's stored entries, y, alpha, mass and N alone; rows
 * longer than SAGE_CSR_MEAN_CHUNK entries are cut into chunks summed apart
 * and added in chunk order; err and mass are per-tile partials added in a fixed
 * order.  No float atomics: two calls on the same inputs give the same bits.
 * Wrong ids give wrong numbers, never an access out of range: ids from col are
 * clamped into [0, N), row pointers into [0, rowptr[N]] and made non-decreasing.
 *
 * sage_pagerank_init   replaces x = 1 / N (nx.pagerank's start): stores x,
 *                      inv_out (from out_degree, or from the row lengths when
 *                      it is NULL), y, state = {0, mass}, and plans the chunk
 *                      split of the rows into the workspace.
 * sage_pagerank_load   the same start from the caller's x and inv_out (neither
 *                      is written): y, state = {0, mass} and the plan.
 * sage_pagerank_step   one iteration; the workspace is the one init / load
 *                      filled for this rowptr (any other gives wrong numbers).
 *                      x_next and y_next are arrays of their own.
 * num_edges bounds rowptr[N] and sizes the workspace, as sage_csr_sum's
 * max_edges does; a step must pass what init passed.
 * Host validation, before any launch: num_nodes outside [1, 2^31), num_edges
 * < 0, alpha outside (0, 1), a NULL array, aliased outputs: SAGE_EINVAL; a
 * short workspace: SAGE_ENOSPACE.  The size query is host arithmetic and
 * returns 0 for a shape out of range.  Workspace 256-byte aligned.
 * ------------------------------------------------------------------------- */
size_t sage_pagerank_workspace_bytes(int64_t num_nodes, int64_t num_edges);
int sage_pagerank_init(const int64_t* rowptr, int64_t num_nodes, int64_t num_edges,
                       const int32_t* out_degree /* [N], nullable = row lengths */,
                       float* x, float* y, float* inv_out, float* state /* [2]: err, mass */,
                       void* workspace, size_t workspace_bytes, sage_stream_t stream);
int sage_pagerank_load(const int64_t* rowptr, int64_t num_nodes, int64_t num_edges,
                       const float* x, const float* inv_out, float* y, float* state,
                       void* workspace, size_t workspace_bytes, sage_stream_t stream);
int sage_pagerank_step(const int64_t* rowptr, const int32_t* col, int64_t num_nodes, int64_t num_edges,
                       const float* inv_out, float alpha, const float* x, const float* y,
                       float* x_next, float* y_next, float* state,
                       void* workspace, size_t workspace_bytes, sage_stream_t stream);

/* ---------------------------------------------------------------------------
 * sage_csr_cheb_* (additive, ABI 9) -- the A.X product of the
 * `eigen_decomposition` initializer.
 * model.py:163-180 (and its two copies) takes LA.eig of the dense adjacency
 * matrix and uses the eigenvectors of the feature_dim largest eigenvalues as
 * the feature table.  ops.eigen_top computes those vectors by Chebyshev-
 * filtered subspace iteration, whose only sparse operation is one step of a
 * three-term recurrence on a block of dim columns, in one pass:
 *     S_i       = sum of y[col[e], :] over e in [rowptr[i], rowptr[i+1])
 *     out[i, :] = fma(a, S_i, fma(b, y[i, :], g * x[i, :]))
 *     out[i, :] = fma(a, S_i, b * y[i, :])                   when x is NULL
 * (a = 1, b = g = 0: the plain product A.y.)  rowptr is int64 [N + 1], col
 * int32 with at least rowptr[N] entries, y, x and out fp32 [N, dim] row-major
 * with leading dimensions ldy, ldx, ldo >= dim.
 * Order of the sums: S_i has the bits of sage_csr_sum -- each column is summed
 * in stored order, rows longer than SAGE_CSR_MEAN_CHUNK entries are cut into
 * chunks summed apart and added in chunk order.  out[i, :] depends on row i's
 * stored entries, y, x[i, :] and the three scalars alone, not on the rows
 * beside it, on dim's cut into lanes or on the grid.  No float atomics: two
 * calls on the same inputs give the same bits.
 * A row is walked by a group of 16, 32 or 64 lanes, the smallest that holds
 * its columns at four per lane (one per lane when dim, a leading dimension or
 * a pointer does not allow 16-byte accesses); wider rows loop over column
 * blocks.
 * Wrong ids give wrong numbers, never an access out of range: ids from col are
 * clamped into [0, N), row pointers into [0, rowptr[N]] and made non-decreasing.
 *
 * sage_csr_cheb_plan   plans the chunk split of the rows into the workspace,
 *                      once per graph.
 * sage_csr_cheb_step   one step; the workspace is the one plan filled for this
 *                      rowptr, num_nodes, num_edges and dim (any other gives
 *                      wrong numbers).  out may be x (with ldo == ldx): a row
 *                      reads only its own row of x before it is stored.  out
 *                      must not overlap y.
 * num_edges bounds rowptr[N] and sizes the workspace, as sage_csr_sum's
 * max_edges does; a step must pass what plan passed.
 * Host validation, before any launch: num_nodes outside [1, 2^31), num_edges
 * < 0, dim outside [1, 2^20], a leading dimension below dim, a NULL array, out
 * overlapping y: SAGE_EINVAL; a short workspace: SAGE_ENOSPACE.  The size query
 * is host arithmetic and returns 0 for a shape out of range.  Workspace
 * 256-byte aligned.
 * ------------------------------------------------------------------------- */
size_t sage_csr_cheb_workspace_bytes(int64_t num_nodes, int64_t num_edges, int32_t dim);
int sage_csr_cheb_plan(const int64_t* rowptr, int64_t num_nodes, int64_t num_edges, int32_t dim,
                       void* workspace, size_t workspace_bytes, sage_stream_t stream);
int sage_csr_cheb_step(const int64_t* rowptr, const int32_t* col, int64_t num_nodes, int64_t num_edges,
                       const float* y, int64_t ldy, const float* x /* nullable */, int64_t ldx, int32_t dim,
                       float a, float b, float g, float* out, int64_t ldo,
                       void* workspace, size_t workspace_bytes, sage_stream_t stream);

/* (ABI 5: sage_set_option is gone with the only option it carried -- the producer / consumer contraction kernel of round 3 was measured
 * slower inside the pipeline and deleted in round 4.) */

#ifdef __cplusplus
}
#endif
#endif /* SAGE355_H */
