"""Whole-graph training: one SGD step of SupervisedGraphSage (model.py:52-69, 240-252) on FULL neighbourhoods
(num_sample=None, aggregators.py:47-48) of every node -- the computation inference.embed_all_nodes serves, differentiated.

The sampled trainer (train.EngineTrainer) draws new neighbour sets every step.  Here nothing is drawn: the loss is a pure
function of the weights, the gradient is exact, and two runs give the same bits (no float atomics anywhere on the path:
sage_csr_mean and sage_csr_mean_backward add in CSR order, sage_linear_act_backward_ws adds its row ranges in range order,
the head adds its 64-row ranges in range order).  The feature table is frozen (model.py:214-215), so the layer-1 mean is a
constant of the graph and is computed once; a step is one csr_mean at width h1, its backward at width h1, two contractions
and their backward kernels.  Single process: data-parallel whole-graph training is not provided.
"""
import time

import numpy as np
import torch
from torch.nn import init

from . import dist, native, ops
from .native import ACT_RELU, SageError
from .train import _sum_over_batch


class FullGraphTrainer:
    """rowptr / col: the CSR of enc1.adj_lists (layer 1), rowptr_outer / col_outer that of enc2.adj_lists (layer 2; default the
    same), as for inference.embed_all_nodes; table [>= N, d0] is frozen.  Weights are initialised in EngineTrainer's order (w1, w2,
    w_cls, xavier_uniform_, dist.broadcast_params): one torch seed gives both trainers the same start.

    Empty rows follow the ZEROS rule (any_nonempty=None), not the reference's per-batch 0/0 = NaN rule: the weight gradients sum
    over all N rows, and a NaN row -- though its own gradient is zero -- would poison every one of them (0 * NaN).  forward() is
    therefore bit-identical to embed_all_nodes(..., nan_empty=False).

    head: "native" -- one sage_xent_head call; "torch" -- the same expressions as stock torch ops (train.EngineTrainer)."""

    def __init__(self, rowptr, col, table, num_classes, hidden1=50, hidden2=128, gcn=True, lr=0.7, agg_self_loop=False, head="native",
                 rowptr_outer=None, col_outer=None):
        if head not in ("torch", "native"):
            raise SageError(f"FullGraphTrainer: head = {head!r}, expected 'torch' or 'native'")
        ops._need_gpu()
        if head == "native" and not ops.xent_head_supported(hidden2, num_classes):
            raise SageError(f"FullGraphTrainer: head='native' has no kernel for hidden2 = {hidden2}, num_classes = {num_classes}")
        ops._chk(rowptr, torch.int64, "rowptr", 1)
        ops._chk(col, torch.int32, "col", 1)
        table, _ = ops._row_major(table, "table")
        self.rowptr, self.col = rowptr, col
        self.rowptr2 = rowptr if rowptr_outer is None else ops._chk(rowptr_outer, torch.int64, "rowptr_outer", 1)
        self.col2 = col if col_outer is None else ops._chk(col_outer, torch.int32, "col_outer", 1)
        if self.rowptr2.shape[0] != rowptr.shape[0]:
            raise SageError("inner and outer CSR must cover the same node ids")
        self.n = rowptr.shape[0] - 1
        if self.n < 1 or table.shape[0] < self.n:
            raise SageError(f"FullGraphTrainer: table has {table.shape[0]} rows for {self.n} nodes")
        self.table = table
        self.head, self.lr, self.concat, self.self_loop = head, float(lr), not gcn, bool(agg_self_loop)
        dev = table.device
        d0 = table.shape[1]
        m = 1 if gcn else 2
        self.d0, self.h1, self.h2 = d0, int(hidden1), int(hidden2)
        self.w1 = torch.empty(hidden1, m * d0, device=dev)
        self.w2 = torch.empty(hidden2, m * hidden1, device=dev)
        self.w_cls = torch.empty(num_classes, hidden2, device=dev)
        for w in (self.w1, self.w2, self.w_cls):
            init.xavier_uniform_(w)
        dist.broadcast_params(self.parameters())
        # the transpose of the layer-2 graph: what csr_mean's backward sums over.  Built once (a sort of the edges)
        self.rowptr2_t, self.col2_t = ops.csr_transpose(self.rowptr2, self.col2)
        self._ws = {}
        self.agg1 = self.h1_out = self.agg2 = self.out = None
        self.refresh_table()

    def parameters(self):
        return [self.w1, self.w2, self.w_cls]

    def _scratch(self, name, nbytes):
        t = self._ws.get(name)
        if t is None or t.numel() < nbytes:
            t = self._ws[name] = torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=self.table.device)
        return t

    def refresh_table(self):
        """The layer-1 mean of the (frozen) table: computed at construction, and again here after the caller changed the table."""
        ws = self._scratch("mean1", ops.csr_mean_workspace_bytes(self.n, self.col.numel(), self.d0))
        self.agg1 = ops.csr_mean(self.rowptr, self.col, self.table, self_loop=self.self_loop, out=self.agg1, workspace=ws)
        return self.agg1

    def forward(self):
        """[N, h2] embeddings of every node; agg1, h1 and agg2 stay in the trainer for the backward."""
        tab = self.table[:self.n]
        self.h1_out = ops.linear_act(self.agg1, self.w1, ACT_RELU, self_tab=tab if self.concat else None, out=self.h1_out)
        ws = self._scratch("mean2", ops.csr_mean_workspace_bytes(self.n, self.col2.numel(), self.h1))
        self.agg2 = ops.csr_mean(self.rowptr2, self.col2, self.h1_out, self_loop=self.self_loop, out=self.agg2, workspace=ws)
        self.out = ops.linear_act(self.agg2, self.w2, ACT_RELU, self_tab=self.h1_out if self.concat else None, out=self.out)
        return self.out

    def _linear_backward(self, self_tab, agg, weight, out, grad_out, need_x, what):
        """sage_linear_act_backward_ws over all N rows -> (grad_weight, grad_x [N, kw] or None)."""
        lib, P = native.lib(), native.ptr
        n, dim = agg.shape
        out_dim, kw = weight.shape
        g_w = torch.zeros_like(weight)
        g_x = torch.empty(n, kw, device=agg.device) if need_x else None
        ws = self._scratch("dw", lib.sage_linear_act_backward_workspace_bytes(n, dim, int(self_tab is not None), out_dim))
        rc = lib.sage_linear_act_backward_ws(P(self_tab), self_tab.stride(0) if self_tab is not None else 0, None, P(agg), agg.stride(0), dim,
                                             P(weight), weight.stride(0), out_dim, ACT_RELU, P(out), out.stride(0), P(grad_out),
                                             grad_out.stride(0), n, None, P(g_w), g_w.stride(0), P(g_x), kw, None,
                                             P(ws), ws.numel(), native.stream_handle())
        native.check(rc, what)
        return g_w, g_x

    def grads(self, train_ids, labels):
        """loss (device scalar) and the gradients of (w1, w2, w_cls) on the training rows; nothing is updated.
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
        if self.head == "native":
            r = ops.xent_head(emb, self.w_cls, labels, scale=1.0 / b, workspace=self._scratch("head", ops.xent_head_workspace_bytes(b, self.h2, self.w_cls.shape[0])))
            loss, g_emb, g_cls = r["loss"][0], r["grad_emb"], r["grad_w"]
        else:
            scores = (emb @ self.w_cls.t()).requires_grad_(True)
            loss = torch.nn.functional.cross_entropy(scores, labels)
            (g_scores,) = torch.autograd.grad(loss, (scores,))
            loss = loss.detach()
            g_emb = g_scores @ self.w_cls                                   # [B, C] x [C, H2]: reduction over the classes
            g_cls = _sum_over_batch(g_scores, emb)                           # [C, B] x [B, H2]: reduction over the batch, fixed order
        g_out = torch.zeros_like(out).index_copy_(0, idx, g_emb)
        # layer 2 over all N rows (a row outside the training set adds exact zeros): dW2 and d[h1_self | agg2]
        g_w2, g_x2 = self._linear_backward(self.h1_out if self.concat else None, self.agg2, self.w2, out, g_out, True, "linear_act_backward (layer 2)")
        ds = self.h1 if self.concat else 0
        ws = self._scratch("mean2_bwd", ops.csr_mean_backward_workspace_bytes(self.n, self.n, self.col2_t.numel(), self.h1))
        g_h1 = ops.csr_mean_backward(self.rowptr2, self.col2, self.rowptr2_t, self.col2_t, g_x2[:, ds:], self_loop=self.self_loop, workspace=ws)
        if self.concat:
            g_h1 += g_x2[:, :ds]                                             # the concat encoder's own-row part
        # layer 1: only dW1, the table is frozen
        g_w1, _ = self._linear_backward(self.table[:self.n] if self.concat else None, self.agg1, self.w1, self.h1_out, g_h1, False,
                                        "linear_act_backward (layer 1)")
        return loss, (g_w1, g_w2, g_cls)

    def step(self, train_ids, labels):
        """forward + backward + in-place SGD; -> the loss as a device scalar (reading it is the caller's only synchronisation)."""
        loss, (g1, g2, gc) = self.grads(train_ids, labels)
        self.w1.add_(g1, alpha=-self.lr)
        self.w2.add_(g2, alpha=-self.lr)
        self.w_cls.add_(gc, alpha=-self.lr)
        return loss

    def predict(self, ids=None):
        """int32 classes of the nodes `ids` (every node without): the class of the highest score (model.py:256)."""
        emb = self.forward()
        if ids is not None:
            emb = emb.index_select(0, ids.long())
        if self.head != "native":
            return (emb @ self.w_cls.t()).argmax(1).to(torch.int32)
        return ops.xent_head(emb, self.w_cls, grads=False, pred=True)["pred"]


def run_full_graph_training(graph, feat_data, labels, num_classes, seed=1, steps=100, lr=0.7, hidden1=50, hidden2=128, gcn=True,
                            agg_self_loop=False, head="native"):
    """run_model (model.py:184-259) with full neighbourhoods: the same 10 / 10 / 80 split of np.random.permutation
    (model.py:229-235), ONE step per epoch over the whole training set, `steps` epochs.
    -> dict(f1_micro, f1_macro, mean_step_time, losses, trainer), as train.run_engine_training."""
    from sklearn.metrics import f1_score
    dev = torch.device("cuda")
    np.random.seed(seed)
    rowptr, col = graph.to(dev)
    table = torch.as_tensor(feat_data, dtype=torch.float32).to(dev)
    n = graph.num_nodes
    rand_indices = np.random.permutation(n)
    val = rand_indices[int(0.1 * n):int(0.2 * n)]
    train = rand_indices[int(0.2 * n):]
    tr = FullGraphTrainer(rowptr, col, table, num_classes, hidden1, hidden2, gcn=gcn, lr=lr, agg_self_loop=agg_self_loop, head=head)
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
    pred = tr.predict(torch.as_tensor(val.astype(np.int32)).to(dev)).cpu().numpy()
    truth = np.asarray(labels)[val].reshape(-1)
    return {"f1_micro": float(f1_score(truth, pred, average="micro")), "f1_macro": float(f1_score(truth, pred, average="macro")),
            "mean_step_time": elapsed / max(int(steps), 1), "losses": [float(x) for x in losses], "trainer": tr}
