"""autograd.Function wrappers: forward = HIP operator, backward = HIP operator.

The reference gets its gradients from stock autograd through mm / div / cat /
relu; here each operator carries its own backward kernel
(include/sage355.h: sage_linear_act_backward, sage_gather_mean_backward, sage_csr_mean_backward, sage_csr_sum,
sage_csr_mean_backward_grouped, sage_csr_mean_backward_rows).
"""
import torch

from . import native, ops


class _GatherMean(torch.autograd.Function):
    @staticmethod
    def forward(ctx, table, nbr, cnt, any_nonempty, slot_rows, self_row):
        out = ops.gather_mean(table, nbr, cnt, slot_rows=slot_rows, self_row=self_row, any_nonempty=any_nonempty)
        ctx.save_for_backward(nbr, cnt, slot_rows, self_row)
        ctx.table_shape = tuple(table.shape)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        nbr, cnt, slot_rows, self_row = ctx.saved_tensors
        grad_table = ops.gather_mean_backward(grad_out.contiguous(), nbr, cnt, ctx.table_shape[0], slot_rows=slot_rows, self_row=self_row)
        return grad_table, None, None, None, None, None


class _CsrMean(torch.autograd.Function):
    """The whole-graph full-neighbourhood mean (ops.csr_mean over every node) and its adjoint (ops.csr_mean_backward)."""

    @staticmethod
    def forward(ctx, table, rowptr, col, rowptr_t, col_t, self_loop, any_nonempty):
        out = ops.csr_mean(rowptr, col, table, self_loop=self_loop, any_nonempty=any_nonempty)
        ctx.save_for_backward(rowptr, col, rowptr_t, col_t)
        ctx.self_loop, ctx.table_rows = self_loop, table.shape[0]
        return out

    @staticmethod
    def backward(ctx, grad_out):
        rowptr, col, rowptr_t, col_t = ctx.saved_tensors
        n = rowptr.shape[0] - 1
        grad_out = grad_out.contiguous()
        if ctx.table_rows == n:
            grad_table = torch.empty((n, grad_out.shape[1]), dtype=torch.float32, device=grad_out.device)
        else:                                             # rows at or past num_nodes belong to no node: zero gradient
            grad_table = torch.zeros((ctx.table_rows, grad_out.shape[1]), dtype=torch.float32, device=grad_out.device)
        ops.csr_mean_backward(rowptr, col, rowptr_t, col_t, grad_out, self_loop=ctx.self_loop, out=grad_table[:n])
        return grad_table, None, None, None, None, None, None


class _CsrMeanIndexed(torch.autograd.Function):
    """The whole-graph mean of embed[index] (ops.csr_mean(index=...)) and its adjoint with respect to the embedding
    (ops.csr_mean_backward_grouped): no [N, dim] array in either direction."""

    @staticmethod
    def forward(ctx, embed, rowptr, col, index, grouped, any_nonempty):
        out = ops.csr_mean(rowptr, col, embed, self_loop=grouped.self_loop, any_nonempty=any_nonempty, index=index)
        ctx.save_for_backward(rowptr, col, grouped.rowptr, grouped.col)
        ctx.self_loop = grouped.self_loop
        return out

    @staticmethod
    def backward(ctx, grad_out):
        rowptr, col, rowptr_gt, col_gt = ctx.saved_tensors
        grouped = ops.GroupedTranspose(rowptr_gt, col_gt, ctx.self_loop)
        return ops.csr_mean_backward_grouped(rowptr, col, grouped, grad_out.contiguous()), None, None, None, None, None


class _CsrMeanRows(torch.autograd.Function):
    """The full-neighbourhood mean of a seed batch (ops.csr_mean(nodes=..., index=...)) and its adjoint with respect to the table
    it reads (ops.csr_mean_backward_rows): the rows may repeat and may share neighbours, nothing [N, dim] is built."""

    @staticmethod
    def forward(ctx, table, rowptr, col, nodes, index, self_loop, any_nonempty, max_edges):
        out = ops.csr_mean(rowptr, col, table, nodes=nodes, self_loop=self_loop, any_nonempty=any_nonempty, index=index,
                           max_edges=max_edges)
        ctx.save_for_backward(rowptr, col, nodes, index)
        ctx.self_loop, ctx.table_rows, ctx.max_edges = self_loop, table.shape[0], max_edges
        return out

    @staticmethod
    def backward(ctx, grad_out):
        rowptr, col, nodes, index = ctx.saved_tensors
        n = rowptr.shape[0] - 1
        rows = ctx.table_rows
        if index is None and rows > n:                    # rows at or past num_nodes belong to no node: zero gradient
            grad_table = torch.zeros((rows, grad_out.shape[1]), dtype=torch.float32, device=grad_out.device)
            ops.csr_mean_backward_rows(rowptr, col, nodes, grad_out.contiguous(), self_loop=ctx.self_loop, out=grad_table[:n],
                                       max_edges=ctx.max_edges)
        else:
            grad_table = ops.csr_mean_backward_rows(rowptr, col, nodes, grad_out.contiguous(), index=index, num_rows=rows,
                                                    self_loop=ctx.self_loop, max_edges=ctx.max_edges)
        return grad_table, None, None, None, None, None, None, None


class _EmbedRows(torch.autograd.Function):
    """weight[index] and its adjoint: row k of the gradient is the sum of the rows that read it (ops.csr_sum over the grouping)."""

    @staticmethod
    def forward(ctx, weight, index, rowptr_g, col_g):
        ctx.save_for_backward(rowptr_g, col_g)
        return weight.index_select(0, index)

    @staticmethod
    def backward(ctx, grad_out):
        rowptr_g, col_g = ctx.saved_tensors
        return ops.csr_sum(rowptr_g, col_g, grad_out.contiguous()), None, None, None


class _LinearAct(torch.autograd.Function):
    @staticmethod
    def forward(ctx, agg, weight, self_tab, self_index, act):
        out = ops.linear_act(agg, weight, act=act, self_tab=self_tab, self_index=self_index)
        ctx.save_for_backward(agg, weight, self_tab, self_index, out)
        ctx.act = act
        return out

    @staticmethod
    def backward(ctx, grad_out):
        agg, weight, self_tab, self_index, out = ctx.saved_tensors
        grad_out = grad_out.contiguous()
        n, dim = agg.shape
        kw = weight.shape[1]
        need_x = ctx.needs_input_grad[0] or (self_tab is not None and ctx.needs_input_grad[2])
        # the reproducible form: partial tiles in a workspace, added in a fixed order (no fp32 atomics)
        grad_w, grad_x = ops.linear_act_backward(agg, weight, ctx.act, out, grad_out, self_tab=self_tab, self_index=self_index,
                                                 need_w=ctx.needs_input_grad[1], need_x=need_x)
        grad_agg = grad_self = None
        if grad_x is not None:
            ds = kw - dim
            if ctx.needs_input_grad[0]:
                grad_agg = grad_x[:, ds:]
            if self_tab is not None and ctx.needs_input_grad[2]:
                gs = grad_x[:, :ds]
                if self_index is None:
                    grad_self = torch.zeros_like(self_tab)
                    grad_self[:n] = gs
                else:
                    grad_self = torch.zeros_like(self_tab).index_add_(0, self_index.long(), gs)
        return grad_agg, grad_w, grad_self, None, None


class _TwoHop(torch.autograd.Function):
    """Two stacked Encoders (model.py:219-222) as ONE differentiable operator: forward = TwoHopEngine.forward (sage_forward2),
    backward = TwoHopEngine.backward_weights on the intermediates that forward left in the engine's workspace.  Inputs are the
    two `weight` Parameters (on any device: their gradients go back to where they live); the raw feature table is frozen
    (model.py:214-215).  Output [B, h2] on the GPU."""

    @staticmethod
    def forward(ctx, w1, w2, engine, ids, key):
        engine.keep_means = True             # backward_weights reads the layer-1 means this forward leaves in the workspace
        out = engine.forward(ids, seed=key)
        ctx.engine, ctx.ids, ctx.key, ctx.generation = engine, ids, key, engine.generation
        ctx.devices = (w1.device, w2.device)
        ctx.save_for_backward(out)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        e = ctx.engine
        (out,) = ctx.saved_tensors
        if e.generation != ctx.generation:
            # another forward has used the workspace since (an evaluation between loss and backward): run this one again --
            # the device sampler is a pure function of (key, node id), so the same sets, rows and h1 come back
            out = e.forward(ctx.ids, seed=ctx.key)
        g1, g2 = e.backward_weights(out, grad_out.to(out.device, torch.float32), need_w1=ctx.needs_input_grad[0])
        g1 = g1.to(ctx.devices[0]) if (g1 is not None and ctx.needs_input_grad[0]) else None
        g2 = g2.to(ctx.devices[1]) if ctx.needs_input_grad[1] else None
        return g1, g2, None, None, None


def two_hop(w1, w2, engine, ids, key):
    return _TwoHop.apply(w1, w2, engine, ids, key)


def gather_mean(table, nbr, cnt, any_nonempty=None, slot_rows=None, self_row=None):
    if torch.is_grad_enabled() and table.requires_grad:
        return _GatherMean.apply(table, nbr, cnt, any_nonempty, slot_rows, self_row)
    return ops.gather_mean(table.detach(), nbr, cnt, slot_rows=slot_rows, self_row=self_row, any_nonempty=any_nonempty)


def csr_mean(rowptr, col, table, transpose=None, self_loop=False, any_nonempty=None, nodes=None, index=None, grouped=None):
    """ops.csr_mean, differentiable with respect to `table` in its whole-graph form (row r = node r).  transpose: the pair
    ops.csr_transpose(rowptr, col) gives; built here if absent (a sort of the edges: build it once per graph and pass it).
    Rows of the table at or past num_nodes get a zero gradient.  With `nodes` and a table that requires grad this raises: a
    row subset with duplicates would need a scatter through duplicate rows; differentiate the whole graph and index the result.
    Without grad mode, or with a table that needs no gradient, it is ops.csr_mean unchanged.
    index: int32 [N] on the device -- `table` is a [K, dim] embedding read as table[index[v]] (ops.csr_mean(index=...)), and the
    gradient is the embedding's, [K, dim] (ops.csr_mean_backward_grouped).  grouped: what
    ops.csr_transpose_grouped(rowptr, col, index, K, self_loop) gives; built here if absent (build it once per graph and pass it).
    Its flag must be `self_loop`."""
    if not (torch.is_grad_enabled() and table.requires_grad):
        return ops.csr_mean(rowptr, col, table.detach(), nodes=nodes, self_loop=self_loop, any_nonempty=any_nonempty, index=index)
    if nodes is not None:
        raise native.SageError("autograd.csr_mean: the differentiable form is the whole-graph one (nodes=None)")
    if index is not None:
        if grouped is None:
            grouped = ops.csr_transpose_grouped(rowptr, col, index, table.shape[0], self_loop)
        if not isinstance(grouped, ops.GroupedTranspose) or grouped.self_loop != bool(self_loop) or grouped.rowptr.shape[0] != table.shape[0] + 1:
            raise native.SageError("autograd.csr_mean: grouped was not built for this embedding and this self_loop")
        return _CsrMeanIndexed.apply(table, rowptr, col, index, grouped, any_nonempty)
    rowptr_t, col_t = ops.csr_transpose(rowptr, col) if transpose is None else transpose
    return _CsrMean.apply(table, rowptr, col, rowptr_t, col_t, bool(self_loop), any_nonempty)


def csr_mean_rows(rowptr, col, table, nodes, index=None, self_loop=False, any_nonempty=None, max_edges=None):
    """ops.csr_mean(rowptr, col, table, nodes=nodes, index=index), differentiable with respect to `table`: row r is the
    full-neighbourhood mean of node nodes[r] (int32 on the device; the rows may repeat and share neighbours), read from `table`
    by node id, or through index (int32 [N]: a frontier's id -> row map, an embedding index) from a [K, dim] table.  The gradient
    is [table.shape[0], dim], ops.csr_mean_backward_rows: the batch's terms in a fixed order, no float atomics, the same bits
    every run.  max_edges: an upper bound on the entries of the rows `nodes` for BOTH directions (a bound below the truth would
    drop terms of the gradient); None reads the count on the host in the backward.  Without grad mode, or with a table that
    needs no gradient, it is the plain operator."""
    if not (torch.is_grad_enabled() and table.requires_grad):
        return ops.csr_mean(rowptr, col, table.detach(), nodes=nodes, self_loop=self_loop, any_nonempty=any_nonempty, index=index,
                            max_edges=max_edges)
    if nodes is None:
        raise native.SageError("autograd.csr_mean_rows: nodes is required (the whole-graph form is autograd.csr_mean)")
    return _CsrMeanRows.apply(table, rowptr, col, nodes, index, bool(self_loop), any_nonempty, max_edges)


def embed_rows(weight, index, groups=None):
    """weight[index] -> [len(index), dim] (the lookup of aggregators.py:70 for a whole graph), differentiable with respect to
    `weight` [K, dim] on the device: the backward is ops.csr_sum over groups = ops.group_rows(index, K) -- no float atomics, the
    same bits every run.  groups is built here if absent (a sort of the index: build it once per graph and pass it).  index:
    int32 / int64 [N], values in [0, K).  Without grad mode, or with a weight that needs no gradient, it is the plain index_select."""
    idx = index.long()
    if not (torch.is_grad_enabled() and weight.requires_grad):
        return weight.detach().index_select(0, idx)
    if not weight.is_cuda or weight.dtype != torch.float32 or weight.dim() != 2:
        raise native.SageError("autograd.embed_rows: weight must be a 2-d fp32 device tensor")
    rowptr_g, col_g = ops.group_rows(index, weight.shape[0]) if groups is None else groups
    if rowptr_g.shape[0] != weight.shape[0] + 1 or col_g.shape[0] != index.shape[0]:
        raise native.SageError("autograd.embed_rows: groups do not have the shape of (weight, index)")
    return _EmbedRows.apply(weight, idx, rowptr_g, col_g)


def linear_act(agg, weight, act, self_tab=None, self_index=None):
    needs = torch.is_grad_enabled() and (agg.requires_grad or weight.requires_grad
                                         or (self_tab is not None and self_tab.requires_grad))
    if needs:
        return _LinearAct.apply(agg, weight, self_tab, self_index, act)
    return ops.linear_act(agg.detach(), weight.detach(), act=act,
                          self_tab=None if self_tab is None else self_tab.detach(), self_index=self_index)
