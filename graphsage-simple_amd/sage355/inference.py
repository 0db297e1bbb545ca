"""Whole-graph, layer-wise inference: embeddings of EVERY node, exact (num_sample=None, aggregators.py:47-48).

Sampled batches recompute layer 1 for every neighbour they share and are still sampled.  Layer-wise inference computes
h1 for all N nodes once (full-neighbourhood mean, sage_csr_mean, then the library's fp32-MFMA contraction, sage_linear_act),
then the output layer for all N nodes from h1.  Row r of every result is node r: the caller's ids, no relabelling.

Memory: h1 [N, h1] + out [N, h2] + one [rows_per_call, max(d0, h1)] block of means + the csr_mean workspace.

The feature table may be stored as torch.bfloat16 (index=None): layer 1's mean reads it through sage_csr_mean_bf16, which widens each
element exactly, so every result is that of table.float() bit for bit at half the table's bytes.  The contraction is not touched:
the concat encoder's own rows are widened in torch, one [rows_per_call, d0] fp32 block at a time.  h1 and every output stay fp32.

embed_nodes is the same computation for a chosen batch of nodes: the frontier of the batch's full neighbourhoods (ops.csr_frontier),
layer 1 for the frontier only, layer 2 for the batch -- the bits of embed_all_nodes(...)[seeds] in memory proportional to the frontier.
"""
import torch
import torch.nn as nn

from . import native, ops
from .native import ACT_RELU, SageError

ROWS_PER_CALL = 1 << 18


def _nonempty_flag(rowptr):
    """int32[1] on the device: this CSR has an edge.  The whole graph is the batch, so this is the reference's per-batch
    0/0 rule (aggregators.py:60-61): an empty row is NaN in a graph with edges, zeros in one without."""
    return (rowptr[-1:] > rowptr[:1]).to(torch.int32)


def _check_index(index, n, rows, what):
    """One range check (a host round trip): sage_linear_act does not clamp self_index."""
    ops._chk(index, torch.int32, "index", 1)
    if index.shape[0] != n:
        raise SageError(f"{what}: index has {index.shape[0]} entries for {n} nodes")
    if n > 0:
        lo, hi = int(index.min()), int(index.max())
        if lo < 0 or hi >= rows:
            raise SageError(f"{what}: index {lo if lo < 0 else hi} outside the embedding's {rows} rows")


def layer_all_nodes(rowptr, col, table, weight, concat, self_loop, act, nan_empty=True, rows_per_call=ROWS_PER_CALL, out=None,
                    _ids=None, _block=None, _workspace=None, index=None):
    """One Encoder.forward (encoders.py:47-62, num_sample=None) for every node of the CSR -> out [N, out_dim].
    table [>= N, dim]; weight [out_dim, dim] (gcn) or [out_dim, 2 * dim] (concat: [self | mean]).
    index: int32 [N] on the device, values in [0, K) (checked once per call) -- table is then a [K, dim] embedding and node v's
    row is table[index[v]] (aggregators.py:68-71), read through the index by the mean and by the concat encoder's own row:
    nothing [N, dim] is allocated, the bits are those of layer_all_nodes(table[index]).
    table may be torch.bfloat16 when index is None: the bits of layer_all_nodes(table.float())."""
    ops._need_gpu()
    ops._chk(rowptr, torch.int64, "rowptr", 1)
    ops._chk(col, torch.int32, "col", 1)
    if index is not None:
        ops.refuse_bf16(table, "layer_all_nodes(index=)")
    table, _ = ops._feature_table(table, "table")
    bf16 = table.dtype == torch.bfloat16
    weight, _ = ops._row_major(weight, "weight")
    n = rowptr.shape[0] - 1
    dim = table.shape[1]
    if index is not None:
        _check_index(index, n, table.shape[0], "layer_all_nodes")
    elif table.shape[0] < n:
        raise SageError(f"layer_all_nodes: table has {table.shape[0]} rows for {n} nodes")
    if weight.shape[1] != dim * (2 if concat else 1):
        raise SageError(f"layer_all_nodes: weight is {tuple(weight.shape)}, table is {dim} wide, concat={bool(concat)}")
    dev = table.device
    if out is None:
        out = torch.empty((n, weight.shape[0]), dtype=torch.float32, device=dev)
    if tuple(out.shape) != (n, weight.shape[0]):
        raise SageError(f"layer_all_nodes: out is {tuple(out.shape)}, expected {(n, weight.shape[0])}")
    if n == 0:
        return out
    rows = max(1, min(int(rows_per_call), n))
    ids = _ids if _ids is not None else torch.arange(n, dtype=torch.int32, device=dev)
    block = _block if _block is not None else torch.empty(rows * dim, dtype=torch.float32, device=dev)
    flag = _nonempty_flag(rowptr) if nan_empty else None
    for r0 in range(0, n, rows):
        r1 = min(r0 + rows, n)
        agg = block[: (r1 - r0) * dim].view(r1 - r0, dim)
        ops.csr_mean(rowptr, col, table, nodes=ids[r0:r1], self_loop=self_loop, any_nonempty=flag, out=agg, workspace=_workspace, index=index)
        if index is None:
            own = (table[r0:r1].float() if bf16 else table[r0:r1]) if concat else None     # bf16: the block's own rows, widened
            ops.linear_act(agg, weight, act, self_tab=own, out=out[r0:r1])
        else:
            ops.linear_act(agg, weight, act, self_tab=table if concat else None, self_index=index[r0:r1] if concat else None, out=out[r0:r1])
    return out


def embed_all_nodes(rowptr, col, table, w1, w2, concat=False, agg_self_loop=False, act1=ACT_RELU, act2=ACT_RELU, nan_empty=True,
                    rowptr_outer=None, col_outer=None, rows_per_call=ROWS_PER_CALL, out=None, index=None):
    """The two-layer stack (model.py:219-222) with num_sample=None at both hops, for every node -> [N, h2].
    Arguments mean what they mean for engine.TwoHopEngine: rowptr/col the CSR of enc1.adj_lists (layer 1),
    rowptr_outer/col_outer that of enc2.adj_lists (layer 2; default the same), w1 [h1, d0 | 2*d0], w2 [h2, h1 | 2*h1].
    index: int32 [N] on the device -- the 1hot / node_degree initializers (aggregators.py:30-31, 68-71): table is the [K, d0]
    embedding and layer 1 reads node v's row as table[index[v]] (layer_all_nodes).  The bits are those of table=table[index]."""
    ops._need_gpu()
    rp2 = rowptr if rowptr_outer is None else rowptr_outer
    c2 = col if col_outer is None else col_outer
    if rp2.shape[0] != rowptr.shape[0]:
        raise SageError("inner and outer CSR must cover the same node ids")
    n = rowptr.shape[0] - 1
    mult = 2 if concat else 1
    h1, h2 = w1.shape[0], w2.shape[0]
    if w1.dim() != 2 or w2.dim() != 2 or w1.shape[1] != mult * table.shape[1] or w2.shape[1] != mult * h1:
        raise SageError(f"weight shapes {tuple(w1.shape)}, {tuple(w2.shape)} do not fit d0={table.shape[1]}, concat={bool(concat)}")
    dev = table.device
    rows = max(1, min(int(rows_per_call), max(n, 1)))
    ids = torch.arange(n, dtype=torch.int32, device=dev)
    block = torch.empty(rows * max(table.shape[1], h1), dtype=torch.float32, device=dev)
    edges = max(col.numel(), c2.numel())
    ws = torch.empty(max(ops.csr_mean_workspace_bytes(rows, edges, max(table.shape[1], h1)), 1), dtype=torch.uint8, device=dev)
    hidden = torch.empty((n, h1), dtype=torch.float32, device=dev)
    layer_all_nodes(rowptr, col, table, w1, concat, agg_self_loop, act1, nan_empty, rows, hidden, ids, block, ws, index=index)
    return layer_all_nodes(rp2, c2, hidden, w2, concat, agg_self_loop, act2, nan_empty, rows, out, ids, block, ws)


def _row_edges(rowptr, ids, live=None):
    """0-d int64 on the device: the edges of rows `ids` (int32 node ids; clamped into the graph, so a bad id reads nothing
    outside rowptr), of the first `live` (a device scalar) of them when given."""
    v = ids.long().clamp_(0, max(rowptr.shape[0] - 2, 0))
    deg = rowptr[v + 1] - rowptr[v]
    if live is not None:
        deg = deg * (torch.arange(ids.shape[0], device=ids.device) < live)
    return deg.sum()


def _seed_frontier(rowptr, rp2, c2, seeds, fr, what):
    """The frontier F of a seed batch into the cleared ops.CsrFrontier `fr`: the distinct ids among `seeds` (int32 on the device, at
    least one) and all their neighbours in the outer CSR (rp2, c2) -> (e2, size, e1): the seeds' outer edges, |F|, and the edges of
    F's rows in the inner CSR `rowptr`.  The caller clears fr afterwards, also when this raises (`what` names it in the messages).
    Two host reads."""
    n, m = rowptr.shape[0] - 1, seeds.shape[0]
    # host read 1: the seeds' outer edges, and their range (device-resident seeds were never checked; sage_linear_act does not clamp)
    e2, lo, hi = torch.stack([_row_edges(rp2, seeds), seeds.min().long(), seeds.max().long()]).tolist()
    if lo < 0 or hi >= n:
        raise SageError(f"{what}: seed id {lo if lo < 0 else hi} outside [0, {n})")
    bound = min(n, m + e2)                                # |F| of a frontier that was empty on entry
    fr.reserve(bound)
    ops.csr_frontier(rp2, c2, seeds, fr, max_edges=e2)
    # host read 2: |F| and the inner edges of F's rows
    size, e1 = torch.stack([fr.count[0].long(), _row_edges(rowptr, fr.nodes[:bound], live=fr.count[0])]).tolist()
    if size > bound:
        if size > fr.max_nodes:                           # overflow: `nodes` no longer names every row of the map
            fr.refill()
        raise SageError(f"{what}: the frontier holds {size} ids, {bound} at most are the seeds': it was not cleared before the call")
    return e2, size, e1


def _layer_rows(rowptr, col, table, weight, concat, self_loop, act, flag, ids, index, self_rows, out, rows, block, workspace, max_edges):
    """layer_all_nodes' block loop for the rows `ids` instead of all of them: out[r] = the layer's output for node ids[r].
    self_rows: the concat encoder's own rows of `table`, one per id.  A bf16 table (index None, so self_rows is ids): the block's own
    rows are gathered and widened in torch and handed over without an index."""
    dim = table.shape[1]
    bf16 = table.dtype == torch.bfloat16
    for r0 in range(0, ids.shape[0], rows):
        r1 = min(r0 + rows, ids.shape[0])
        agg = block[: (r1 - r0) * dim].view(r1 - r0, dim)
        ops.csr_mean(rowptr, col, table, nodes=ids[r0:r1], self_loop=self_loop, any_nonempty=flag, out=agg, max_edges=max_edges,
                     workspace=workspace, index=index)
        if concat and bf16:
            ops.linear_act(agg, weight, act, self_tab=table.index_select(0, ids[r0:r1]).float(), out=out[r0:r1])
        else:
            ops.linear_act(agg, weight, act, self_tab=table if concat else None, self_index=self_rows[r0:r1] if concat else None, out=out[r0:r1])


def embed_nodes(rowptr, col, table, w1, w2, seeds, concat=False, agg_self_loop=False, act1=ACT_RELU, act2=ACT_RELU, nan_empty=True,
                rowptr_outer=None, col_outer=None, rows_per_call=ROWS_PER_CALL, index=None, frontier=None, out=None):
    """The two-layer stack with num_sample=None at both hops (aggregators.py:47-48) for the nodes `seeds` only -> [len(seeds), h2],
    row r = node seeds[r]: embed_all_nodes(the same arguments)[seeds] BIT FOR BIT, without computing any other row.  seeds: list /
    numpy / tensor of ids, may repeat, may be empty; an id outside the graph raises SageError.
    F, the distinct ids among the seeds and all their OUTER neighbours (ops.csr_frontier), gets layer 1 in blocks of rows_per_call
    into a compact h1_F [|F|, h1]; layer 2 is the indexed mean of the seeds' outer rows with the frontier's id -> row map as its index
    (the set-union self term is still decided on node ids).  The NaN flag of each layer is that of its WHOLE CSR, as embed_all_nodes
    passes it.  Every row's arithmetic is csr_mean's and linear_act's for that row, which depend on neither the row's position nor
    the rows beside it: hence the bits, whatever order F comes in.
    frontier: an ops.CsrFrontier of this graph, cleared, to reuse its [N] map (default: one is built, an O(N) fill); it is cleared
    again before returning, also when an error follows the kernel.
    Host reads: two per call -- the edge count of the seeds' rows (with the seeds' range), then |F| with F's inner edge count; they
    size the frontier, h1_F and the csr_mean workspaces (never len(col): that would be a workspace for the whole graph).
    Memory: the map (4 N bytes, or the caller's), h1_F, out, one [rows_per_call, max(d0, h1)] block of means.
    table may be torch.bfloat16 when index is None: the bits of embed_nodes(table.float()); the concat encoder then adds one
    [rows_per_call, d0] fp32 block of own rows, never an [N, d0] array."""
    ops._need_gpu()
    rp2 = rowptr if rowptr_outer is None else rowptr_outer
    c2 = col if col_outer is None else col_outer
    ops._chk(rowptr, torch.int64, "rowptr", 1)
    ops._chk(rp2, torch.int64, "rowptr_outer", 1)
    if rp2.shape[0] != rowptr.shape[0]:
        raise SageError("inner and outer CSR must cover the same node ids")
    n = rowptr.shape[0] - 1
    mult = 2 if concat else 1
    if index is not None:
        ops.refuse_bf16(table, "embed_nodes(index=)")
    table, _ = ops._feature_table(table, "table")
    d0, h1, h2 = table.shape[1], w1.shape[0], w2.shape[0]
    if w1.dim() != 2 or w2.dim() != 2 or w1.shape[1] != mult * d0 or w2.shape[1] != mult * h1:
        raise SageError(f"weight shapes {tuple(w1.shape)}, {tuple(w2.shape)} do not fit d0={d0}, concat={bool(concat)}")
    if index is not None:
        _check_index(index, n, table.shape[0], "embed_nodes")
    elif table.shape[0] < n:
        raise SageError(f"embed_nodes: table has {table.shape[0]} rows for {n} nodes")
    if frontier is not None and (not isinstance(frontier, ops.CsrFrontier) or frontier.num_nodes != n):
        raise SageError(f"embed_nodes: frontier must be an ops.CsrFrontier of {n} nodes")
    dev = table.device
    seeds = ops.as_ids(seeds, dev, num_nodes=n)
    if seeds.dim() != 1:
        raise SageError("embed_nodes: seeds must be one-dimensional")
    m = seeds.shape[0]
    if out is None:
        out = torch.empty((m, h2), dtype=torch.float32, device=dev)
    if tuple(out.shape) != (m, h2):
        raise SageError(f"embed_nodes: out is {tuple(out.shape)}, expected {(m, h2)}")
    if m == 0:
        return out
    fr = ops.CsrFrontier(n, dev, max_nodes=0) if frontier is None else frontier
    try:
        e2, size, e1 = _seed_frontier(rowptr, rp2, c2, seeds, fr, "embed_nodes")
        f_nodes = fr.nodes[:size]
        rows = max(1, min(int(rows_per_call), max(size, m)))
        block = torch.empty(rows * max(d0, h1), dtype=torch.float32, device=dev)
        ws = torch.empty(max(ops.csr_mean_workspace_bytes(min(rows, size), e1, d0), ops.csr_mean_workspace_bytes(min(rows, m), e2, h1), 1),
                         dtype=torch.uint8, device=dev)
        h1_f = torch.empty((size, h1), dtype=torch.float32, device=dev)
        self1 = (f_nodes if index is None else index[f_nodes.long()]) if concat else None
        _layer_rows(rowptr, col, table, w1, concat, agg_self_loop, act1, _nonempty_flag(rowptr) if nan_empty else None, f_nodes, index,
                    self1, h1_f, rows, block, ws, e1)
        self2 = fr.pos[seeds.long()] if concat else None
        _layer_rows(rp2, c2, h1_f, w2, concat, agg_self_loop, act2, _nonempty_flag(rp2) if nan_empty else None, seeds, fr.pos,
                    self2, out, rows, block, ws, e2)
    finally:
        fr.clear()
    return out


def _module_tensor(t, what):
    if not isinstance(t, torch.Tensor):
        raise SageError(f"{what}: not a tensor")
    return t.detach().to("cuda", torch.float32).contiguous()


def _first_one_index(weight, embed_rows, block_elems=1 << 24):
    """int32 [N] on the device: the position of the first element equal to 1 in every row of the one-hot feature table
    (aggregators.py:68-69), taken on the device in row blocks of about block_elems elements -- the table is never held twice.
    A row without a 1 (the reference's IndexError) and an index past the embedding's rows raise."""
    n, width = weight.shape
    index = torch.empty(n, dtype=torch.int32, device="cuda")
    rows = max(1, block_elems // max(width, 1))
    ok = torch.ones((), dtype=torch.bool, device="cuda")
    for r0 in range(0, n, rows):
        is_one = weight[r0:r0 + rows].detach().to("cuda") == 1
        ok &= is_one.any(1).all()
        index[r0:r0 + rows] = is_one.to(torch.int8).argmax(1)       # of equal maxima argmax returns the first
    if n > 0 and not bool(ok):
        raise SageError("embed_all_from_modules: a feature row holds no element equal to 1")
    if n > 0 and int(index.max()) >= embed_rows:
        raise SageError(f"embed_all_from_modules: index {int(index.max())} outside the embedding's {embed_rows} rows")
    return index


def _stack_arguments(enc2, what, table_dtype=torch.float32):
    """What embed_all_from_modules and embed_nodes_from_modules read from a two-layer stack, with their refusals (`what` names the
    caller in the messages): -> ((rowptr, col, table, w1, w2), keyword arguments) of embed_all_nodes / embed_nodes.
    table_dtype: torch.float32, or torch.bfloat16 = the feature table is rounded once, here, and read as bf16."""
    if table_dtype not in (torch.float32, torch.bfloat16):
        raise SageError(f"{what}: table_dtype {table_dtype}, expected torch.float32 or torch.bfloat16")
    from .aggregators import EMBED_INITIALIZERS, MeanAggregator
    from .encoders import SIGMOID_INITIALIZERS
    from .graph import csr_from_adj_lists

    enc1 = getattr(enc2, "base_model", None)
    if enc1 is None or not hasattr(enc1, "adj_lists") or not hasattr(enc1, "weight"):
        raise SageError(f"{what}: enc2 has no Encoder as base_model")
    if not getattr(enc2, "fuse_base_model", True):
        raise SageError(f"{what}: enc2.fuse_base_model=False declares a feature function other than its base model")
    if not isinstance(enc1.features, nn.Embedding):
        raise SageError(f"{what}: enc1.features is not an nn.Embedding feature table")
    for enc in (enc1, enc2):
        if not isinstance(enc.aggregator, MeanAggregator) and type(enc.aggregator).__name__ != "MeanAggregator":
            raise SageError(f"{what}: aggregator {type(enc.aggregator).__name__} is not a MeanAggregator")
    if isinstance(enc2.initializer, str) and enc2.initializer in EMBED_INITIALIZERS:
        raise SageError(f"{what}: the {enc2.initializer!r} initializer on the outer encoder is not supported")
    detour = isinstance(enc1.initializer, str) and enc1.initializer in EMBED_INITIALIZERS
    if detour:
        if not isinstance(getattr(enc1.aggregator, "embed", None), nn.Embedding):
            raise SageError(f"{what}: initializer {enc1.initializer!r}, but enc1's aggregator was built without it: no `embed`")
        if not enc1.gcn:
            raise SageError(f"{what}: the concat encoder with the {enc1.initializer!r} initializer is not supported")
        if table_dtype == torch.bfloat16:
            raise SageError(f"{what}: table_dtype torch.bfloat16 with the {enc1.initializer!r} initializer: the trained embedding stays fp32")
    if bool(enc1.gcn) != bool(enc2.gcn):
        raise SageError(f"{what}: the two encoders differ in `gcn`")
    agg_gcn = bool(getattr(enc1.aggregator, "gcn", False))
    if agg_gcn != bool(getattr(enc2.aggregator, "gcn", False)):
        raise SageError(f"{what}: the two aggregators differ in `gcn`")

    def act(enc):
        return ops.ACT_SIGMOID if enc.initializer in SIGMOID_INITIALIZERS else ops.ACT_RELU

    with torch.no_grad():
        index = None
        if detour:
            table = _module_tensor(enc1.aggregator.embed.weight, "enc1.aggregator.embed.weight")
            index = _first_one_index(enc1.features.weight, table.shape[0])
            n = index.shape[0]
        else:
            if table_dtype == torch.bfloat16:
                table = enc1.features.weight.detach().to("cuda").to(torch.bfloat16).contiguous()
            else:
                table = _module_tensor(enc1.features.weight, "enc1.features.weight")
            n = table.shape[0]
        w1, w2 = _module_tensor(enc1.weight, "enc1.weight"), _module_tensor(enc2.weight, "enc2.weight")
        g1 = csr_from_adj_lists(enc1.adj_lists, num_nodes=n)
        rp1, c1 = g1.to("cuda")
        rp2, c2 = (rp1, c1) if enc2.adj_lists is enc1.adj_lists else csr_from_adj_lists(enc2.adj_lists, num_nodes=n).to("cuda")
        return (rp1, c1, table, w1, w2), dict(concat=not enc1.gcn, agg_self_loop=agg_gcn, act1=act(enc1), act2=act(enc2), nan_empty=True,
                                              rowptr_outer=rp2, col_outer=c2, index=index)


def embed_all_from_modules(enc2, rows_per_call=ROWS_PER_CALL, table_dtype=torch.float32):
    """embed_all_nodes on a trained two-layer stack as model.py:214-222 wires it (this package's Encoder / MeanAggregator, or
    the reference's classes of the same shape): enc1 = enc2.base_model over an nn.Embedding feature table.  Reads the table,
    both `weight` Parameters, the encoders' `gcn` flag, the aggregators' `gcn` flag, the activations (the initializer rule)
    and both adj_lists (each converted to CSR once per call).  -> device tensor [N, h2], row r = node r.
    A layer-1 encoder with the "1hot" / "node_degree" initializer (gcn form): the feature table's rows are one-hots that index the
    trainable enc1.aggregator.embed (aggregators.py:30-31, 68-71); index[v] is the position of the first 1 of row v, the embedding
    is read through it (embed_all_nodes(index=...)), and nothing [N, embed_dim] is built.  Refused: a row without a 1, an index
    past the embedding's rows, an aggregator without `embed`, the concat encoder with such an initializer (the reference feeds
    the raw one-hot as the own row there, fullgraph.py), and such an initializer on enc2.
    table_dtype=torch.bfloat16: enc1.features.weight is rounded to bf16 once per call and layer 1 reads that (embed_all_nodes);
    refused with the embedding initializers.
    Anything else raises SageError."""
    args, kwargs = _stack_arguments(enc2, "embed_all_from_modules", table_dtype)
    return embed_all_nodes(*args, rows_per_call=rows_per_call, **kwargs)


def embed_nodes_from_modules(enc2, nodes, rows_per_call=ROWS_PER_CALL, table_dtype=torch.float32):
    """embed_nodes on the stack embed_all_from_modules takes, with its argument extraction and its refusals:
    -> device tensor [len(nodes), h2], row r = node nodes[r], the bits of embed_all_from_modules(enc2)[nodes]."""
    args, kwargs = _stack_arguments(enc2, "embed_nodes_from_modules", table_dtype)
    return embed_nodes(*args, nodes, rows_per_call=rows_per_call, **kwargs)
