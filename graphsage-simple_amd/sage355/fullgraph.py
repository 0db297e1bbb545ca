"""Whole-graph training: one SGD step of SupervisedGraphSage (model.py:52-69, 240-252) on FULL neighbourhoods
(num_sample=None, aggregators.py:47-48) of every node -- the computation inference.embed_all_nodes serves, differentiated.

The sampled trainer (train.EngineTrainer) draws new neighbour sets every step.  Here nothing is drawn: the loss is a pure
function of the weights, the gradient is exact, and two runs give the same bits (no float atomics anywhere on the path:
sage_csr_mean and sage_csr_mean_backward add in CSR order, sage_linear_act_backward_ws adds its row ranges in range order,
the head adds its 64-row ranges in range order).  The feature table is frozen (model.py:214-215), so the layer-1 mean is a
constant of the graph and is computed once; a step is one csr_mean at width h1, its backward at width h1, two contractions
and their backward kernels.  Single process: data-parallel whole-graph training is not provided.

Featureless graphs (the reference's `--initializer 1hot | node_degree`, aggregators.py:30-31, 68-71): layer 1 reads rows of a
TRAINABLE embedding instead of the table, X = embed[index] with index[v] = v (1hot) or the degree of v (node_degree).  The
layer-1 mean is then part of every step, its backward is sage_csr_mean_backward at width embed_dim on the inner graph, and the
embedding's gradient is the sum of the rows of all nodes that share an embedding row: sage_csr_sum over the grouping of the
index (ops.group_rows), dense and in a fixed order -- still no float atomics, still the same bits every run.

fused_embed=True keeps X out of memory: the layer-1 mean reads embed[index[col[e]]] (sage_csr_mean_indexed, the same bits), the
concat encoder's own row is read through the index, and the embedding's gradient is summed straight onto its rows
(sage_csr_mean_backward_grouped over ops.csr_transpose_grouped's list) with no [N, embed_dim] gradient of X in between.  That sum
adds the unfused path's terms in another association: equal to rounding, not to the bit, and as reproducible.
"""
import time

import numpy as np
import torch

from . import dist, ops
from .head import head_grads, head_predict
from .native import ACT_RELU, ACT_SIGMOID, SageError
from .train import _split, _validation_result, check_trainer_args, csr_pair, init_parameters


class FullGraphTrainer:
    """rowptr / col: the CSR of enc1.adj_lists (layer 1), rowptr_outer / col_outer that of enc2.adj_lists (layer 2; default the
    same), as for inference.embed_all_nodes; table [>= N, d0] is frozen.  Weights are initialised as EngineTrainer's are
    (train.init_parameters, then dist.broadcast_params): one torch seed gives both trainers the same start.

    Empty rows follow the ZEROS rule (any_nonempty=None), not the reference's per-batch 0/0 = NaN rule: the weight gradients sum
    over all N rows, and a NaN row -- though its own gradient is zero -- would poison every one of them (0 * NaN).  forward() is
    therefore bit-identical to embed_all_nodes(..., nan_empty=False).

    head: "native" -- one sage_xent_head call; "torch" -- the same expressions as stock torch ops (train.EngineTrainer).

    table may be torch.bfloat16 with gcn=True, a storage format: refresh_table's mean widens it exactly (sage_csr_mean_bf16), the
    backward never reads the table, and every result is that of table.float() bit for bit.  The concat encoder is refused: its own
    rows would need the [N, d0] fp32 copy that a bf16 table exists to avoid (ExactBatchTrainer widens a batch's own rows instead).

    Trainable embedding: embed_index int32 [N] on the device with values in [0, embed_rows), and table=None.  Layer 1 reads
    X = embed[embed_index] ([N, embed_dim]); self.embed [embed_rows, embed_dim] is drawn N(0, 1) as nn.Embedding's weight is
    (aggregators.py:31), AFTER w1, w2, w_cls -- one torch seed still gives those three the start the frozen-table trainer gives them --
    is broadcast with them, is the fourth of parameters() and of grads()'s gradients, and is updated by step().  act1: layer 1's
    activation, ACT_RELU or ACT_SIGMOID (encoders.py:58 applies the sigmoid for node_degree).  The concat encoder's own row is X[v];
    the reference's concat form feeds the raw one-hot feature row there instead (encoders.py:51-54), which would need a weight as
    wide as the one-hot: that form is not provided.  forward() is bit-identical to
    embed_all_nodes(table=embed[embed_index], act1=act1, nan_empty=False).  When embed_index is arange(N) with embed_rows == N, X is
    the embedding itself: no copy, and its gradient needs no csr_sum.

    fused_embed (default False; read only with a non-identity embed_index): layer 1 reads the embedding through the index in
    both directions and X = embed[embed_index] is never built (self.x stays None).  forward(), the loss and the gradients of w2
    and w_cls keep their bits; the embedding's gradient is the same sum in another association (one flat sequence per embedding
    row, csr_mean_backward_grouped; for concat plus csr_sum of the own-row part)."""

    def __init__(self, rowptr, col, table, num_classes, hidden1=50, hidden2=128, gcn=True, lr=0.7, agg_self_loop=False, head="native",
                 rowptr_outer=None, col_outer=None, embed_index=None, embed_rows=None, embed_dim=None, act1=ACT_RELU, fused_embed=False):
        check_trainer_args("FullGraphTrainer", head, act1, hidden2, num_classes, table, embed_index, embed_rows, embed_dim)
        ops._need_gpu()
        self.rowptr, self.col = rowptr, col
        self.rowptr2, self.col2 = csr_pair(rowptr, col, rowptr_outer, col_outer)
        self.n = rowptr.shape[0] - 1
        if embed_index is None:
            table, _ = ops._feature_table(table, "table")
            if table.dtype == torch.bfloat16 and not gcn:
                raise SageError("FullGraphTrainer: a torch.bfloat16 table with the concat encoder (gcn=False) is not supported: its own rows "
                                "would need an [N, d0] fp32 copy of the table; use gcn=True, ExactBatchTrainer, or table.float()")
            if self.n < 1 or table.shape[0] < self.n:
                raise SageError(f"FullGraphTrainer: table has {table.shape[0]} rows for {self.n} nodes")
            dev, d0 = table.device, table.shape[1]
        else:
            ops._chk(embed_index, torch.int32, "embed_index", 1)
            if self.n < 1 or embed_index.shape[0] != self.n:
                raise SageError(f"FullGraphTrainer: embed_index has {embed_index.shape[0]} entries for {self.n} nodes")
            dev, d0 = embed_index.device, int(embed_dim)
        self.table, self.embed_index, self.dev = table, embed_index, dev
        self.head, self.lr, self.concat, self.self_loop, self.act1 = head, float(lr), not gcn, bool(agg_self_loop), act1
        self.d0, self.h1, self.h2 = d0, int(hidden1), int(hidden2)
        self.w1, self.w2, self.w_cls, self.embed = init_parameters(dev, d0, hidden1, hidden2, num_classes, gcn,
                                                                   None if embed_index is None else embed_rows)
        dist.broadcast_params(self.parameters())
        # the transpose of the layer-2 graph: what csr_mean's backward sums over.  Built once (a sort of the edges)
        self.rowptr2_t, self.col2_t = ops.csr_transpose(self.rowptr2, self.col2)
        self.scratch = ops.Scratch(dev)
        self.agg1 = self.h1_out = self.agg2 = self.out = self.x = None
        self.fused = False
        if embed_index is None:
            self.refresh_table()
            return
        # what the embedding's backward sums over, both built once: the transpose of the layer-1 graph (the outer one's when there
        # is one graph), and the nodes of every embedding row (group_rows refuses an index outside [0, embed_rows))
        one_graph = self.rowptr2 is rowptr and self.col2 is col
        self.rowptr_t, self.col_t = (self.rowptr2_t, self.col2_t) if one_graph else ops.csr_transpose(rowptr, col)
        self.identity = int(embed_rows) == self.n and bool(torch.equal(embed_index, torch.arange(self.n, dtype=torch.int32, device=dev)))
        self.groups = None if self.identity else ops.group_rows(embed_index, int(embed_rows))
        self.fused = bool(fused_embed) and not self.identity
        self._index64 = None if (self.identity or self.fused) else embed_index.long()
        # the fused gradient's list: every embedding row's terms in one sequence (built once; it carries self_loop)
        self.grouped_t = ops.csr_transpose_grouped(rowptr, col, embed_index, int(embed_rows), self.self_loop) if self.fused else None

    def parameters(self):
        return [self.w1, self.w2, self.w_cls] + ([self.embed] if self.embed is not None else [])

    def refresh_table(self):
        """The layer-1 mean of the (frozen) table: computed at construction, and again here after the caller changed the table.
        With a trainable embedding there is no table to refresh: the mean is computed by every forward()."""
        if self.embed is not None:
            raise SageError("FullGraphTrainer.refresh_table: layer 1 reads a trainable embedding, not a table")
        ws = self.scratch.get("mean1", ops.csr_mean_workspace_bytes(self.n, self.col.numel(), self.d0))
        self.agg1 = ops.csr_mean(self.rowptr, self.col, self.table, self_loop=self.self_loop, out=self.agg1, workspace=ws)
        return self.agg1

    def forward(self):
        """[N, h2] embeddings of every node; agg1, h1 and agg2 stay in the trainer for the backward."""
        self_index = None
        if self.embed is None:
            tab = self.table[:self.n]
        elif self.fused:                                     # X = embed[embed_index] is read through the index, never built
            tab, self_index = self.embed, self.embed_index
            ws = self.scratch.get("mean1", ops.csr_mean_workspace_bytes(self.n, self.col.numel(), self.d0))
            self.agg1 = ops.csr_mean(self.rowptr, self.col, tab, self_loop=self.self_loop, out=self.agg1, workspace=ws, index=self_index)
        else:
            tab = self.x = self.embed if self.identity else torch.index_select(self.embed, 0, self._index64, out=self.x)
            ws = self.scratch.get("mean1", ops.csr_mean_workspace_bytes(self.n, self.col.numel(), self.d0))
            self.agg1 = ops.csr_mean(self.rowptr, self.col, tab, self_loop=self.self_loop, out=self.agg1, workspace=ws)
        self.h1_out = ops.linear_act(self.agg1, self.w1, self.act1, self_tab=tab if self.concat else None,
                                     self_index=self_index if self.concat else None, out=self.h1_out)
        ws = self.scratch.get("mean2", ops.csr_mean_workspace_bytes(self.n, self.col2.numel(), self.h1))
        self.agg2 = ops.csr_mean(self.rowptr2, self.col2, self.h1_out, self_loop=self.self_loop, out=self.agg2, workspace=ws)
        self.out = ops.linear_act(self.agg2, self.w2, ACT_RELU, self_tab=self.h1_out if self.concat else None, out=self.out)
        return self.out

    def grads(self, train_ids, labels):
        """loss (device scalar) and the gradients of (w1, w2, w_cls) -- and of embed, fourth, when layer 1 reads a trainable
        embedding -- on the training rows; nothing is updated.
        train_ids: DISTINCT int32 node ids on the device, labels int64 [len(train_ids)].  The rows' gradients are placed with
        index_copy_ (distinct ids: no two writers), never with an atomic scatter."""
        ops._chk(train_ids, torch.int32, "train_ids", 1)
        ops._chk(labels, torch.int64, "labels", 1)
        b = train_ids.shape[0]
        if b < 1 or labels.shape[0] != b:
            raise SageError(f"FullGraphTrainer.grads: {b} training ids, {labels.shape[0]} labels")
        out = self.forward()
        idx = train_ids.long()
        emb = out.index_select(0, idx)
        ws = self.scratch.get("head", ops.xent_head_workspace_bytes(b, self.h2, self.w_cls.shape[0])) if self.head == "native" else None
        loss, g_emb, g_cls = head_grads(emb, self.w_cls, labels, self.head, b, workspace=ws)
        g_out = torch.zeros_like(out).index_copy_(0, idx, g_emb)
        # layer 2 over all N rows (a row outside the training set adds exact zeros): dW2 and d[h1_self | agg2]
        dw = self.scratch.get("dw", max(ops.linear_act_backward_workspace_bytes(self.n, self.h1, self.concat, self.h2),
                                        ops.linear_act_backward_workspace_bytes(self.n, self.d0, self.concat, self.h1)))
        g_w2, g_x2 = ops.linear_act_backward(self.agg2, self.w2, ACT_RELU, out, g_out, self_tab=self.h1_out if self.concat else None, workspace=dw)
        ds = self.h1 if self.concat else 0
        ws = self.scratch.get("mean2_bwd", ops.csr_mean_backward_workspace_bytes(self.n, self.n, self.col2_t.numel(), self.h1))
        g_h1 = ops.csr_mean_backward(self.rowptr2, self.col2, self.rowptr2_t, self.col2_t, g_x2[:, ds:], self_loop=self.self_loop, workspace=ws)
        if self.concat:
            g_h1 += g_x2[:, :ds]                                             # the concat encoder's own-row part
        if self.embed is None:                                               # layer 1: only dW1, the table is frozen
            g_w1, _ = ops.linear_act_backward(self.agg1, self.w1, self.act1, self.h1_out, g_h1, need_x=False, workspace=dw,
                                              self_tab=self.table[:self.n] if self.concat else None)
            return loss, (g_w1, g_w2, g_cls)
        if self.fused:
            # layer 1 through the index: dW1 and d[X_self | agg1]; every embedding row then sums its terms of the mean's adjoint in
            # one sequence, and for concat the own-row parts of the nodes that read it (ascending node order) on top
            g_w1, g_x1 = ops.linear_act_backward(self.agg1, self.w1, self.act1, self.h1_out, g_h1, workspace=dw,
                                                 self_tab=self.embed if self.concat else None, self_index=self.embed_index if self.concat else None)
            ds = self.d0 if self.concat else 0
            k = self.embed.shape[0]
            ws = self.scratch.get("mean1_bwd", ops.csr_mean_backward_grouped_workspace_bytes(self.n, k, self.grouped_t.col.numel(), self.d0))
            g_embed = ops.csr_mean_backward_grouped(self.rowptr, self.col, self.grouped_t, g_x1[:, ds:], workspace=ws)
            if self.concat:
                rowptr_g, col_g = self.groups
                ws = self.scratch.get("embed_sum", ops.csr_sum_workspace_bytes(k, self.n, self.d0))
                g_embed += ops.csr_sum(rowptr_g, col_g, g_x1[:, :ds], workspace=ws)
            return loss, (g_w1, g_w2, g_cls, g_embed)
        # layer 1 with its input's gradient: dW1 and d[X_self | agg1]; the mean's adjoint on the inner graph gives dX
        g_w1, g_x1 = ops.linear_act_backward(self.agg1, self.w1, self.act1, self.h1_out, g_h1, self_tab=self.x if self.concat else None,
                                             workspace=dw)
        ds = self.d0 if self.concat else 0
        ws = self.scratch.get("mean1_bwd", ops.csr_mean_backward_workspace_bytes(self.n, self.n, self.col_t.numel(), self.d0))
        g_x = ops.csr_mean_backward(self.rowptr, self.col, self.rowptr_t, self.col_t, g_x1[:, ds:], self_loop=self.self_loop, workspace=ws)
        if self.concat:
            g_x += g_x1[:, :ds]                                              # the concat encoder's own-row part
        if self.identity:
            return loss, (g_w1, g_w2, g_cls, g_x)
        # every embedding row collects the rows of the nodes that read it, in ascending node order
        rowptr_g, col_g = self.groups
        ws = self.scratch.get("embed_sum", ops.csr_sum_workspace_bytes(rowptr_g.shape[0] - 1, self.n, self.d0))
        return loss, (g_w1, g_w2, g_cls, ops.csr_sum(rowptr_g, col_g, g_x, workspace=ws))

    def step(self, train_ids, labels):
        """forward + backward + in-place SGD; -> the loss as a device scalar (reading it is the caller's only synchronisation)."""
        loss, g = self.grads(train_ids, labels)
        for w, gw in zip(self.parameters(), g):
            w.add_(gw, alpha=-self.lr)
        return loss

    def predict(self, ids=None):
        """int32 classes of the nodes `ids` (every node without): the class of the highest score (model.py:256)."""
        emb = self.forward()
        if ids is not None:
            emb = emb.index_select(0, ids.long())
        return head_predict(emb, self.w_cls, self.head)


def one_hot_index(n, device="cuda"):
    """(index, K) of the 1hot initializer: node v reads embedding row v, K = n rows."""
    return torch.arange(int(n), dtype=torch.int32, device=device), int(n)


def degree_index(rowptr):
    """(index, K) of the node_degree initializer (model.py:153-157): node v reads the row of its layer-1 degree len(adj_lists[v])
    -- its CSR row's length -- and K = max degree + 1.  rowptr: int64 [N + 1], on any device; the index lives beside it."""
    deg = (rowptr[1:] - rowptr[:-1]).to(torch.int32)
    return deg.contiguous(), (int(deg.max()) + 1 if deg.numel() else 1)


def check_table_dtype(who, table_dtype, trainable_embedding):
    """The table_dtype argument of a run driver `who`: torch.float32, or torch.bfloat16 for a frozen table only."""
    if table_dtype not in (torch.float32, torch.bfloat16):
        raise SageError(f"{who}: table_dtype = {table_dtype!r}, expected torch.float32 or torch.bfloat16")
    if table_dtype == torch.bfloat16 and trainable_embedding:
        raise SageError(f"{who}: table_dtype torch.bfloat16 with a trainable embedding: bf16 stores a frozen table, the embedding stays fp32")
    return table_dtype


def embed_arguments(who, initializer, frozen, graph, embed_dim, dev, act1=None):
    """What a run driver `who` hands its trainer for --initializer (model.py:153-157, 209-212): None for a spelling in `frozen` (the
    frozen feature table), else dict(embed_index, embed_rows, embed_dim, act1) -- "1hot": a row per node, ReLU; "node_degree": a row
    per degree, SIGMOID at layer 1 (encoders.py:58-59).  Anything else is refused, before the graph is read.
    act1: the driver's own act1 argument, which belongs to a frozen table (frozen_arguments); with an initializer that sets layer
    1's activation itself it is refused."""
    if initializer not in (*frozen, "1hot", "node_degree"):
        raise SageError(f"{who}: initializer = {initializer!r}, expected {frozen[0]!r}, '1hot' or 'node_degree'")
    if initializer in frozen:
        return None
    if act1 is not None:
        raise SageError(f"{who}: act1 = {act1!r} with initializer = {initializer!r}, which sets layer 1's activation itself; act1 goes "
                        "with a frozen table (datasets.pagerank_table with ACT_SIGMOID)")
    if initializer == "1hot":
        index, rows = one_hot_index(graph.num_nodes, dev)
    else:
        index, rows = degree_index(torch.from_numpy(graph.rowptr))
    return dict(embed_index=index.to(dev), embed_rows=rows, embed_dim=embed_dim, act1=ACT_SIGMOID if initializer == "node_degree" else ACT_RELU)


def frozen_arguments(act1):
    """What a run driver hands the trainer of a frozen table for its act1 argument: None is the trainer's own default (ReLU); a
    table that wants another layer-1 activation names it -- datasets.pagerank_table goes with ACT_SIGMOID (encoders.py:58)."""
    return {} if act1 is None else dict(act1=act1)


def run_full_graph_training(graph, feat_data, labels, num_classes, seed=1, steps=100, lr=0.7, hidden1=50, hidden2=128, gcn=True,
                            agg_self_loop=False, head="native", initializer="None", embed_dim=100, fused_embed=False,
                            table_dtype=torch.float32, act1=None):
    """run_model (model.py:184-259) with full neighbourhoods: the same 10 / 10 / 80 split of a seeded numpy permutation
    (model.py:229-235), ONE step per epoch over the whole training set, `steps` epochs.
    initializer: "None" -- the frozen table feat_data, ReLU at both layers; "1hot" -- a trainable embedding row per node, ReLU;
    "node_degree" -- a trainable embedding row per degree, SIGMOID at layer 1 (encoders.py:58).  feat_data is not read for the
    last two and may be None.  embed_dim is the embedding's width; its default is the reference's --feature_dim default.  The
    reference itself overrides that width for these two initializers with the one-hot's (N and max degree + 1, model.py:209-212)
    because its loader hands the one-hot in as the feature table: an accident of the loader, not copied here.
    fused_embed: FullGraphTrainer's flag (it changes something for "node_degree" only: the 1hot index is the identity).
    table_dtype: torch.float32, or torch.bfloat16 = the frozen table is rounded to bf16 once and stored so (gcn=True only; refused
    with a trainable embedding).
    act1: layer 1's activation over a frozen table (None: ReLU), ACT_SIGMOID for datasets.pagerank_table; refused with an initializer.
    -> dict(f1_micro, f1_macro, mean_step_time, losses, trainer), as train.run_engine_training."""
    dev = torch.device("cuda")
    embed = embed_arguments("run_full_graph_training", initializer, ("None",), graph, embed_dim, dev, act1)
    table_dtype = check_table_dtype("run_full_graph_training", table_dtype, embed is not None)
    rowptr, col = graph.to(dev)
    _, val, train = _split(graph.num_nodes, seed)
    table = torch.as_tensor(feat_data, dtype=torch.float32).to(dev).to(table_dtype) if embed is None else None
    tr = FullGraphTrainer(rowptr, col, table, num_classes, hidden1, hidden2, gcn=gcn, lr=lr, agg_self_loop=agg_self_loop, head=head,
                          fused_embed=fused_embed, **(embed or frozen_arguments(act1)))
    labels_dev = torch.as_tensor(np.asarray(labels).reshape(-1), dtype=torch.int64).to(dev)
    ids = torch.as_tensor(train.astype(np.int32)).to(dev)
    tgt = labels_dev[ids.long()]
    losses = []
    torch.cuda.synchronize()
    t0 = time.time()
    for _ in range(int(steps)):
        losses.append(tr.step(ids, tgt))
    torch.cuda.synchronize()
    elapsed = time.time() - t0
    pred = tr.predict(torch.as_tensor(val.astype(np.int32)).to(dev))
    return _validation_result(labels, val, pred, elapsed, int(steps), losses, tr)
