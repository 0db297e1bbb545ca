"""Exact mini-batch training: one SGD step of SupervisedGraphSage (model.py:52-69, 240-252) on a SEED BATCH embedded from the FULL
neighbourhoods of its nodes (num_sample=None, aggregators.py:47-48) -- the computation inference.embed_nodes serves, differentiated.

fullgraph.FullGraphTrainer differentiates the same expression for every node and touches all N rows in every step, however small the
training batch.  Here a step costs what the batch's two-hop neighbourhood costs: the frontier F of the seeds' outer rows
(ops.csr_frontier), layer 1 for the |F| rows, layer 2 for the seeds through the frontier's id -> row map, and backwards the adjoint of
that indexed mean with respect to the compact h1_F (ops.csr_mean_backward_rows).  No float array has N rows; the trainer owns one
int32 [N] map.  Nothing is drawn, the gradient is exact, and two runs give the same bits: no float atomics anywhere on the path.
ExactBatchTrainer's feature table is frozen (model.py:214-215); ExactBatchEmbedTrainer trains featureless graphs (the reference's
`--initializer 1hot | node_degree`, aggregators.py:30-31, 68-71): layer 1 reads a trainable embedding through an index, and the
layer-1 mean gets a batch adjoint as well -- dense (ops.csr_mean_backward_rows over the embedding's rows) or, for tables of millions
of rows, for the touched rows only with the SGD update fused in (ops.csr_mean_backward_touched).  Single process.
"""
import random
import time

import numpy as np
import torch

from . import dist, ops
from .head import head_grads, head_predict
from .fullgraph import check_table_dtype, embed_arguments, frozen_arguments
from .inference import _check_index, _seed_frontier
from .native import ACT_RELU, SageError
from .train import _batches, _split, _validation_result, check_trainer_args, csr_pair, init_parameters


class ExactBatchTrainer:
    """The frozen-table form of FullGraphTrainer for seed batches: the same arguments, the weights w1, w2, w_cls drawn by the same
    train.init_parameters (one torch seed gives both trainers the same start), the ZEROS rule for empty rows, the same two heads.

    forward(seeds) is bit-identical to embed_nodes(..., nan_empty=False) and to FullGraphTrainer.forward()[seeds]; the loss and the
    gradient of w_cls of grads(seeds, labels) are bit-identical to FullGraphTrainer.grads(seeds, labels) (the head sees the same rows
    in the same order); the gradients of w1 and w2 are the same sums over fewer rows in another association: equal to rounding.

    seeds: DISTINCT int32 node ids on the device, as FullGraphTrainer.grads requires of train_ids (the concat encoder's own-row
    gradient is placed with index_copy_, never with an atomic scatter).  An id outside the graph raises.
    Host reads per step: embed_nodes' two (the seeds' outer edge count with their range; |F| with F's inner edge count).
    The trainer owns one persistent ops.CsrFrontier; its map is cleared after the backward has read it, also when a step raises.
    The frontier's rows are put in ascending id order before layer 1 runs, so two runs of a step give the same bits.

    table may be torch.bfloat16, a storage format: the caller rounded it once, layer 1's mean widens it exactly (sage_csr_mean_bf16),
    and everything a step computes is what it computes on table.float().  The concat encoder widens the frontier's own rows once per
    step ([|F|, d0] fp32) and hands them to the contraction and its backward as they are, without an index."""

    def __init__(self, rowptr, col, table, num_classes, hidden1=50, hidden2=128, gcn=True, lr=0.7, agg_self_loop=False, head="native",
                 rowptr_outer=None, col_outer=None, act1=ACT_RELU):
        check_trainer_args("ExactBatchTrainer", head, act1, hidden2, num_classes)
        ops._need_gpu()
        self.rowptr, self.col = rowptr, col
        self.rowptr2, self.col2 = csr_pair(rowptr, col, rowptr_outer, col_outer)
        table, _ = ops._feature_table(table, "table")
        self.n = rowptr.shape[0] - 1
        if self.n < 1 or table.shape[0] < self.n:
            raise SageError(f"ExactBatchTrainer: table has {table.shape[0]} rows for {self.n} nodes")
        self.table = table
        self._start(table.device, table.shape[1], num_classes, hidden1, hidden2, gcn, lr, agg_self_loop, head, act1)

    def _start(self, dev, d0, num_classes, hidden1, hidden2, gcn, lr, agg_self_loop, head, act1, embed_rows=None):
        """What both trainers set up once layer 1's input is known: the options, the parameters (train.init_parameters' draw order,
        then the broadcast), the frontier and the scratch."""
        self.dev = dev
        self.head, self.lr, self.concat, self.self_loop, self.act1 = head, float(lr), not gcn, bool(agg_self_loop), act1
        self.d0, self.h1, self.h2 = int(d0), int(hidden1), int(hidden2)
        self.w1, self.w2, self.w_cls, self.embed = init_parameters(dev, self.d0, hidden1, hidden2, num_classes, gcn, embed_rows)
        dist.broadcast_params(self.parameters())
        self.frontier = ops.CsrFrontier(self.n, dev, max_nodes=0)
        self.scratch = ops.Scratch(dev)

    def parameters(self):
        return [self.w1, self.w2, self.w_cls]

    def _layer1(self):
        """(table, index) that layer 1 reads: node v's row is table[v], or table[index[v]] with an index."""
        return self.table, None

    def _forward(self, seeds):
        """The forward of one batch; the frontier's map stays FILLED for the backward (the callers clear it in a finally).
        -> dict of what the backward reads: the frontier's nodes, the seeds' rows, layer 1's own rows (self1: their rows of the table;
        own1, own1_index: what the contraction reads them through), agg1, h1_F, agg2, out and the two edge counts."""
        ops._chk(seeds, torch.int32, "seeds", 1)
        m, fr, who = seeds.shape[0], self.frontier, type(self).__name__
        if m < 1:
            raise SageError(f"{who}: no seeds")
        e2, size, e1 = _seed_frontier(self.rowptr, self.rowptr2, self.col2, seeds, fr, who)
        # The frontier hands its rows out in whatever order its waves won them.  The rows' values do not depend on that, but dW1 adds
        # the rows up in row order: put F in ascending id order (|F| integers sorted, the map rewritten), so that a step's bits
        # depend on the seeds alone.
        f_nodes = fr.nodes[:size]
        f_nodes.copy_(torch.sort(f_nodes).values)
        fr.pos.index_copy_(0, f_nodes.long(), torch.arange(size, dtype=torch.int32, device=self.dev))
        ws = self.scratch.get("mean", max(ops.csr_mean_workspace_bytes(size, e1, self.d0), ops.csr_mean_workspace_bytes(m, e2, self.h1)))
        tab, index = self._layer1()
        self1 = (f_nodes if index is None else index[f_nodes.long()]) if self.concat else None     # the concat encoder's own rows of tab
        agg1 = ops.csr_mean(self.rowptr, self.col, tab, nodes=f_nodes, self_loop=self.self_loop, max_edges=e1, workspace=ws, index=index)
        own1, own1_index = (tab, self1) if self.concat else (None, None)
        if self.concat and tab.dtype == torch.bfloat16:                # the frontier's own rows, widened once for the forward and the backward
            own1, own1_index = tab.index_select(0, f_nodes).float(), None
        h1_f = ops.linear_act(agg1, self.w1, self.act1, self_tab=own1, self_index=own1_index)
        agg2 = ops.csr_mean(self.rowptr2, self.col2, h1_f, nodes=seeds, self_loop=self.self_loop, max_edges=e2, workspace=ws, index=fr.pos)
        rows = fr.pos[seeds.long()] if self.concat else None           # the seeds' rows of h1_F
        out = ops.linear_act(agg2, self.w2, ACT_RELU, self_tab=h1_f if self.concat else None, self_index=rows)
        return dict(f_nodes=f_nodes, rows=rows, self1=self1, own1=own1, own1_index=own1_index, agg1=agg1, h1_f=h1_f, agg2=agg2, out=out, e2=e2, e1=e1)

    def forward(self, seeds):
        """[len(seeds), h2] embeddings of the nodes `seeds` (int32 on the device; here they may repeat)."""
        try:
            return self._forward(seeds)["out"]
        finally:
            self.frontier.clear()

    def grads(self, seeds, labels):
        """loss (device scalar) and the gradients of (w1, w2, w_cls) on the batch; nothing is updated.
        seeds: DISTINCT int32 node ids on the device, labels int64 [len(seeds)]."""
        return self._grads(seeds, labels)

    def _layer1_grads(self, f, g_h1, dw, update):
        """Layer 1's backward over the frontier's rows -> (g_w1, the gradients of further parameters): only dW1 here, the table is
        frozen."""
        g_w1, _ = ops.linear_act_backward(f["agg1"], self.w1, self.act1, f["h1_f"], g_h1, self_tab=f["own1"], self_index=f["own1_index"],
                                          need_x=False, workspace=dw)
        return g_w1, ()

    def _grads(self, seeds, labels, update=False):
        """grads(); update: a subclass may apply a parameter's update inside its gradient call (_layer1_grads)."""
        ops._chk(seeds, torch.int32, "seeds", 1)
        ops._chk(labels, torch.int64, "labels", 1)
        b = seeds.shape[0]
        if b < 1 or labels.shape[0] != b:
            raise SageError(f"{type(self).__name__}.grads: {b} seeds, {labels.shape[0]} labels")
        try:
            f = self._forward(seeds)
            emb = f["out"]                                   # row r = node seeds[r]: what FullGraphTrainer selects out of its [N, h2]
            ws = self.scratch.get("head", ops.xent_head_workspace_bytes(b, self.h2, self.w_cls.shape[0])) if self.head == "native" else None
            loss, g_emb, g_cls = head_grads(emb, self.w_cls, labels, self.head, b, workspace=ws)
            size = f["f_nodes"].shape[0]
            dw = self.scratch.get("dw", max(ops.linear_act_backward_workspace_bytes(b, self.h1, self.concat, self.h2),
                                            ops.linear_act_backward_workspace_bytes(size, self.d0, self.concat, self.h1)))
            # layer 2 over the seed rows: dW2 and d[h1_self | agg2]
            g_w2, g_x2 = ops.linear_act_backward(f["agg2"], self.w2, ACT_RELU, emb, g_emb, self_tab=f["h1_f"] if self.concat else None,
                                                 self_index=f["rows"], workspace=dw)
            ds = self.h1 if self.concat else 0
            ws = self.scratch.get("mean2_bwd", ops.csr_mean_backward_rows_workspace_bytes(b, f["e2"], size, self.h1))
            g_h1 = ops.csr_mean_backward_rows(self.rowptr2, self.col2, seeds, g_x2[:, ds:], index=self.frontier.pos, num_rows=size,
                                              self_loop=self.self_loop, max_edges=f["e2"], workspace=ws)
            if self.concat:                                  # the own-row part, onto the seeds' rows of h1_F: distinct, so no two writers
                rows = f["rows"].long()
                g_h1.index_copy_(0, rows, g_h1.index_select(0, rows) + g_x2[:, :ds])
            g_w1, more = self._layer1_grads(f, g_h1, dw, update)
            return loss, (g_w1, g_w2, g_cls, *more)
        finally:
            self.frontier.clear()

    def step(self, seeds, labels):
        """forward + backward + in-place SGD; -> the loss as a device scalar."""
        loss, g = self.grads(seeds, labels)
        for w, gw in zip(self.parameters(), g):
            w.add_(gw, alpha=-self.lr)
        return loss

    def predict(self, ids):
        """int32 classes of the nodes `ids` (int32 on the device): the class of the highest score (model.py:256)."""
        emb = self.forward(ids)
        return head_predict(emb, self.w_cls, self.head)


class ExactBatchEmbedTrainer(ExactBatchTrainer):
    """ExactBatchTrainer for featureless graphs (aggregators.py:30-31, 68-71): layer 1 reads the TRAINABLE self.embed [embed_rows,
    embed_dim] through embed_index (int32 [N] on the device, values in [0, embed_rows): fullgraph.one_hot_index / degree_index), and
    X = embed[embed_index] is never built -- still no float array with N rows.  FullGraphTrainer(embed_index=...)'s rules: self.embed
    is drawn N(0, 1) AFTER w1, w2, w_cls (one torch seed gives all four the start that trainer gives them), is broadcast with them and is
    the fourth of parameters() and of grads()'s gradients; act1 is ACT_RELU or ACT_SIGMOID (node_degree, encoders.py:58); the concat
    encoder's own row is embed[embed_index[v]].  forward(seeds) is bit-identical to embed_nodes(table=embed, index=embed_index,
    act1=act1, nan_empty=False), hence to FullGraphTrainer(embed_index=...).forward()[seeds]; loss and the gradient of w_cls are that
    trainer's bits, the other gradients the same sums over fewer rows in another association.

    The embedding's gradient is the batch adjoint of the layer-1 indexed mean: ops.csr_mean_backward_rows over the frontier's rows
    with the embedding index, dense [embed_rows, embed_dim].  The concat encoder's own-row parts are added in a fixed order
    (index_copy_ for an identity index, ops.group_rows + ops.csr_sum otherwise, where rows repeat): no float atomics.
    sparse_embed=True (gcn only; the default stays False): for 1hot tables of millions of rows.  grads() returns the compact triple
    (rows, num_rows, grad_rows) of ops.csr_mean_backward_touched as its fourth entry -- bit for bit the dense gradient's rows -- and
    step() applies the embedding's update inside that call (embed[e] = fma(-lr, g[e], embed[e]) for the touched rows, one
    rounding) without returning a gradient: no array of embed_rows rows exists in a step."""

    def __init__(self, rowptr, col, num_classes, embed_index, embed_rows, embed_dim, hidden1=50, hidden2=128, gcn=True, lr=0.7,
                 agg_self_loop=False, head="native", rowptr_outer=None, col_outer=None, act1=ACT_RELU, sparse_embed=False):
        who = "ExactBatchEmbedTrainer"
        if embed_index is None:
            raise SageError(f"{who}: embed_index is required (ExactBatchTrainer trains on a frozen table)")
        check_trainer_args(who, head, act1, hidden2, num_classes, None, embed_index, embed_rows, embed_dim)
        if sparse_embed and not gcn:
            raise SageError(f"{who}: sparse_embed is not provided with the concat encoder (gcn=False): its own-row gradient is dense")
        ops._need_gpu()
        self.rowptr, self.col = rowptr, col
        self.rowptr2, self.col2 = csr_pair(rowptr, col, rowptr_outer, col_outer)
        self.n = rowptr.shape[0] - 1
        ops._chk(embed_index, torch.int32, "embed_index", 1)
        if self.n < 1 or embed_index.shape[0] != self.n:
            raise SageError(f"{who}: embed_index has {embed_index.shape[0]} entries for {self.n} nodes")
        self.embed_rows = int(embed_rows)
        _check_index(embed_index, self.n, self.embed_rows, who)      # once: sage_linear_act does not clamp the own rows
        self.table, self.embed_index, self.sparse_embed = None, embed_index, bool(sparse_embed)
        self.identity = self.embed_rows == self.n and bool(torch.equal(embed_index, torch.arange(self.n, dtype=torch.int32,
                                                                                                  device=embed_index.device)))
        self._start(embed_index.device, embed_dim, num_classes, hidden1, hidden2, gcn, lr, agg_self_loop, head, act1, self.embed_rows)

    def parameters(self):
        return [self.w1, self.w2, self.w_cls, self.embed]

    def _layer1(self):
        return self.embed, self.embed_index

    def _layer1_grads(self, f, g_h1, dw, update):
        """dW1 and d[X_self | agg1] over the frontier's rows, then the embedding's gradient: every embedding row sums its terms of the
        layer-1 mean's batch adjoint in one sequence."""
        g_w1, g_x1 = ops.linear_act_backward(f["agg1"], self.w1, self.act1, f["h1_f"], g_h1, self_tab=self.embed if self.concat else None,
                                             self_index=f["self1"], workspace=dw)
        ds = self.d0 if self.concat else 0
        f_nodes, size, rows = f["f_nodes"], f["f_nodes"].shape[0], self.embed_rows
        if self.sparse_embed:
            ws = self.scratch.get("mean1_bwd", ops.csr_mean_backward_touched_workspace_bytes(size, f["e1"], rows, self.d0))
            sgd = dict(table=self.embed, lr=self.lr, want_grad=False) if update else {}
            return g_w1, (ops.csr_mean_backward_touched(self.rowptr, self.col, f_nodes, g_x1[:, ds:], index=self.embed_index, num_rows=rows,
                                                        self_loop=self.self_loop, max_edges=f["e1"], workspace=ws, **sgd),)
        ws = self.scratch.get("mean1_bwd", ops.csr_mean_backward_rows_workspace_bytes(size, f["e1"], rows, self.d0))
        g_embed = ops.csr_mean_backward_rows(self.rowptr, self.col, f_nodes, g_x1[:, ds:], index=self.embed_index, num_rows=rows,
                                             self_loop=self.self_loop, max_edges=f["e1"], workspace=ws)
        if self.concat and self.identity:                    # the own-row parts, onto the frontier's own rows: distinct, so no two writers
            own = f_nodes.long()
            g_embed.index_copy_(0, own, g_embed.index_select(0, own) + g_x1[:, :ds])
        elif self.concat:                                    # rows repeat (node_degree): each embedding row adds its nodes' parts in
            rowptr_g, col_g = ops.group_rows(f["self1"], rows)       # ascending frontier-row order
            ws = self.scratch.get("embed_sum", ops.csr_sum_workspace_bytes(rows, size, self.d0))
            g_embed += ops.csr_sum(rowptr_g, col_g, g_x1[:, :ds], workspace=ws)
        return g_w1, (g_embed,)

    def step(self, seeds, labels):
        """forward + backward + in-place SGD; -> the loss as a device scalar.  sparse_embed: the embedding's touched rows are updated
        inside the gradient call, which then returns no gradient."""
        if not self.sparse_embed:
            return super().step(seeds, labels)
        loss, g = self._grads(seeds, labels, update=True)
        for w, gw in zip(self.parameters()[:3], g[:3]):
            w.add_(gw, alpha=-self.lr)
        return loss


def run_exact_batch_training(graph, feat_data, labels, num_classes, seed=1, epochs=1, batch_size=128, ref_batching=False, lr=0.7,
                             hidden1=50, hidden2=128, gcn=True, agg_self_loop=False, head="native", table_dtype=torch.float32, act1=None,
                             initializer="None", embed_dim=100, sparse_embed=False):
    """run_model (model.py:184-259) with num_sample=None batches: the same split, shuffles, batching and SGD as
    train.run_engine_training, every step through ExactBatchTrainer, validation by its predict (full neighbourhoods as well).
    initializer, embed_dim: run_full_graph_training's -- "None": the frozen table feat_data; "1hot" / "node_degree": a trainable
    embedding through ExactBatchEmbedTrainer (feat_data is not read and may be None), with its sparse_embed.
    table_dtype: torch.float32, or torch.bfloat16 = the frozen table is rounded to bf16 once and stored so (half its bytes; exact for
    0/1 features); refused with a trainable embedding, which stays fp32.
    act1: run_full_graph_training's (a frozen table's layer-1 activation; refused with an initializer).
    -> dict(f1_micro, f1_macro, mean_step_time, losses, trainer), as train.run_engine_training."""
    dev = torch.device("cuda")
    embed = embed_arguments("run_exact_batch_training", initializer, ("None",), graph, embed_dim, dev, act1)
    table_dtype = check_table_dtype("run_exact_batch_training", table_dtype, embed is not None)
    if sparse_embed and embed is None:
        raise SageError("run_exact_batch_training: sparse_embed needs initializer '1hot' or 'node_degree': a frozen table has no update")
    rowptr, col = graph.to(dev)
    _, val, train = _split(graph.num_nodes, seed)
    common = dict(hidden1=hidden1, hidden2=hidden2, gcn=gcn, lr=lr, agg_self_loop=agg_self_loop, head=head)
    if embed is None:
        tr = ExactBatchTrainer(rowptr, col, torch.as_tensor(feat_data, dtype=torch.float32).to(dev).to(table_dtype), num_classes, **common,
                               **frozen_arguments(act1))
    else:
        tr = ExactBatchEmbedTrainer(rowptr, col, num_classes, sparse_embed=sparse_embed, **embed, **common)
    labels_dev = torch.as_tensor(np.asarray(labels).reshape(-1), dtype=torch.int64).to(dev)
    losses = []
    torch.cuda.synchronize()
    t0 = time.time()
    for ids in _batches(list(train), random.Random(seed), epochs, batch_size, ref_batching, dev):
        losses.append(tr.step(ids, labels_dev[ids.long()]))
    torch.cuda.synchronize()
    elapsed = time.time() - t0
    pred = tr.predict(torch.as_tensor(val.astype(np.int32)).to(dev))
    return _validation_result(labels, val, pred, elapsed, len(losses), losses, tr)
