"""Whole-graph, layer-wise inference: embeddings of EVERY node, exact (num_sample=None, aggregators.py:47-48).

Sampled batches recompute layer 1 for every neighbour they share and are still sampled.  Layer-wise inference computes
h1 for all N nodes once (full-neighbourhood mean, sage_csr_mean, then the library's fp32-MFMA contraction, sage_linear_act),
then the output layer for all N nodes from h1.  Row r of every result is node r: the caller's ids, no relabelling.

Memory: h1 [N, h1] + out [N, h2] + one [rows_per_call, max(d0, h1)] block of means + the csr_mean workspace.
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
    nothing [N, dim] is allocated, the bits are those of layer_all_nodes(table[index])."""
    ops._need_gpu()
    ops._chk(rowptr, torch.int64, "rowptr", 1)
    ops._chk(col, torch.int32, "col", 1)
    table, _ = ops._row_major(table, "table")
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
            ops.linear_act(agg, weight, act, self_tab=table[r0:r1] if concat else None, out=out[r0:r1])
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


def embed_all_from_modules(enc2, rows_per_call=ROWS_PER_CALL):
    """embed_all_nodes on a trained two-layer stack as model.py:214-222 wires it (this package's Encoder / MeanAggregator, or
    the reference's classes of the same shape): enc1 = enc2.base_model over an nn.Embedding feature table.  Reads the table,
    both `weight` Parameters, the encoders' `gcn` flag, the aggregators' `gcn` flag, the activations (the initializer rule)
    and both adj_lists (each converted to CSR once per call).  -> device tensor [N, h2], row r = node r.
    A layer-1 encoder with the "1hot" / "node_degree" initializer (gcn form): the feature table's rows are one-hots that index the
    trainable enc1.aggregator.embed (aggregators.py:30-31, 68-71); index[v] is the position of the first 1 of row v, the embedding
    is read through it (embed_all_nodes(index=...)), and nothing [N, embed_dim] is built.  Refused: a row without a 1, an index
    past the embedding's rows, an aggregator without `embed`, the concat encoder with such an initializer (the reference feeds
    the raw one-hot as the own row there, fullgraph.py), and such an initializer on enc2.
    Anything else raises SageError."""
    from .aggregators import EMBED_INITIALIZERS, MeanAggregator
    from .encoders import SIGMOID_INITIALIZERS
    from .graph import csr_from_adj_lists

    enc1 = getattr(enc2, "base_model", None)
    if enc1 is None or not hasattr(enc1, "adj_lists") or not hasattr(enc1, "weight"):
        raise SageError("embed_all_from_modules: enc2 has no Encoder as base_model")
    if not getattr(enc2, "fuse_base_model", True):
        raise SageError("embed_all_from_modules: enc2.fuse_base_model=False declares a feature function other than its base model")
    if not isinstance(enc1.features, nn.Embedding):
        raise SageError("embed_all_from_modules: enc1.features is not an nn.Embedding feature table")
    for enc in (enc1, enc2):
        if not isinstance(enc.aggregator, MeanAggregator) and type(enc.aggregator).__name__ != "MeanAggregator":
            raise SageError(f"embed_all_from_modules: aggregator {type(enc.aggregator).__name__} is not a MeanAggregator")
    if isinstance(enc2.initializer, str) and enc2.initializer in EMBED_INITIALIZERS:
        raise SageError(f"embed_all_from_modules: the {enc2.initializer!r} initializer on the outer encoder is not supported")
    detour = isinstance(enc1.initializer, str) and enc1.initializer in EMBED_INITIALIZERS
    if detour:
        if not isinstance(getattr(enc1.aggregator, "embed", None), nn.Embedding):
            raise SageError(f"embed_all_from_modules: initializer {enc1.initializer!r}, but enc1's aggregator was built without it: no `embed`")
        if not enc1.gcn:
            raise SageError(f"embed_all_from_modules: the concat encoder with the {enc1.initializer!r} initializer is not supported")
    if bool(enc1.gcn) != bool(enc2.gcn):
        raise SageError("embed_all_from_modules: the two encoders differ in `gcn`")
    agg_gcn = bool(getattr(enc1.aggregator, "gcn", False))
    if agg_gcn != bool(getattr(enc2.aggregator, "gcn", False)):
        raise SageError("embed_all_from_modules: the two aggregators differ in `gcn`")

    def act(enc):
        return ops.ACT_SIGMOID if enc.initializer in SIGMOID_INITIALIZERS else ops.ACT_RELU

    with torch.no_grad():
        index = None
        if detour:
            table = _module_tensor(enc1.aggregator.embed.weight, "enc1.aggregator.embed.weight")
            index = _first_one_index(enc1.features.weight, table.shape[0])
            n = index.shape[0]
        else:
            table = _module_tensor(enc1.features.weight, "enc1.features.weight")
            n = table.shape[0]
        w1, w2 = _module_tensor(enc1.weight, "enc1.weight"), _module_tensor(enc2.weight, "enc2.weight")
        g1 = csr_from_adj_lists(enc1.adj_lists, num_nodes=n)
        rp1, c1 = g1.to("cuda")
        rp2, c2 = (rp1, c1) if enc2.adj_lists is enc1.adj_lists else csr_from_adj_lists(enc2.adj_lists, num_nodes=n).to("cuda")
        return embed_all_nodes(rp1, c1, table, w1, w2, concat=not enc1.gcn, agg_self_loop=agg_gcn, act1=act(enc1), act2=act(enc2),
                               nan_empty=True, rowptr_outer=rp2, col_outer=c2, rows_per_call=rows_per_call, index=index)
