"""The classifier head of SupervisedGraphSage (model.py:59-69, 249, 256) on given embeddings, for every trainer: scores =
emb . w_cls^T, CrossEntropyLoss, the gradients of both operands, and the predicted class.  head = "native": one sage_xent_head
call, its sums in an order fixed by the shape; head = "torch": the same expressions as stock torch ops.
"""
import torch

from . import ops


def _sum_over_batch(g_scores, emb, piece=256):
    """g_scores^T . emb = [C, B] x [B, H] with the reduction over B in a FIXED order: 256-row pieces as one batched product, their
    sum over the piece index by torch.sum (one thread per output element adds them in index order), a ragged tail last."""
    b = g_scores.shape[0]
    whole = (b // piece) * piece
    if whole <= piece:
        return g_scores.t() @ emb
    n = whole // piece
    acc = torch.bmm(g_scores[:whole].view(n, piece, -1).transpose(1, 2), emb[:whole].view(n, piece, -1)).sum(0)
    if whole < b:
        acc = acc + g_scores[whole:].t() @ emb[whole:]
    return acc


def head_grads(emb, w_cls, labels, head, batch, global_batch=None, workspace=None, out=None):
    """-> (loss, g_emb, g_cls): the loss of `batch` rows of embeddings as a device scalar, d loss / d emb and d loss / d w_cls.
    global_batch: data parallel -- the rows are a shard of a mini-batch of that many seeds; the loss is the SUM over the shard /
    global_batch, so that the SUM of the ranks' gradients is the full-batch gradient.
    workspace, out: the native head's (ops.xent_head); with `out` the three results are views of the caller's buffers."""
    if head == "native":
        # classifier + loss + their gradients in one call: no autograd, and the sum over the batch runs in 64-row ranges added in range
        # order, so w_cls keeps its run-to-run bit identity at any batch size
        r = ops.xent_head(emb, w_cls, labels, scale=1.0 / float(batch if global_batch is None else global_batch), workspace=workspace, out=out)
        return r["loss"][0], r["grad_emb"], r["grad_w"]
    # The classifier's weight gradient is a [C, B] x [B, H2] product whose reduction runs over the BATCH: for B >= 1024 the BLAS behind
    # torch.mm may split it and add the pieces with atomics, and two runs of one schedule then differ in the last bits of w_cls (seen
    # once in four runs of the GPU suite, 1024-seed case only).  So autograd stops at the scores and the two small products are
    # spelled out; the one over the batch is cut into 256-row pieces (one batched product) that are added in a fixed order.
    # (Accumulating it in fp64 instead costs 0.2 ms per step: 0.31 -> 0.53 ms captured at config-3 size.)
    emb, w_cls = emb.detach(), w_cls.detach()
    scores = (emb @ w_cls.t()).requires_grad_(True)
    if global_batch is None:
        loss = torch.nn.functional.cross_entropy(scores, labels)
    else:
        loss = torch.nn.functional.cross_entropy(scores, labels, reduction="sum") / float(global_batch)
    (g_scores,) = torch.autograd.grad(loss, (scores,))
    g_emb = g_scores @ w_cls                                              # [B, C] x [C, H2]: reduction over the classes
    return loss.detach(), g_emb, _sum_over_batch(g_scores, emb)           # [C, B] x [B, H2]: reduction over the batch, fixed order


def head_predict(emb, w_cls, head, workspace=None, out=None):
    """int32 [B]: the class of the highest score (model.py:256, `val_output.data.numpy().argmax(axis=1)`).  The native head computes it
    from the embeddings in one launch (the inference form of sage_xent_head; workspace, out: its arguments); the torch head takes
    the argmax of the scores."""
    if head != "native":
        return (emb @ w_cls.t()).argmax(1).to(torch.int32)
    return ops.xent_head(emb, w_cls, grads=False, pred=True, workspace=workspace, out=out)["pred"]
