"""Training / evaluation harness: this build's counterpart of graphsage/model.py:52-69
(SupervisedGraphSage) and model.py:184-259 (run_model) -- SURVEY.md section 8 row f-1.

Kept from the reference: the classifier (weight [C, embed_dim], xavier, scores = (W . embeds)^T,
CrossEntropyLoss), the 10 / 10 / 80 test / val / train split of a seeded numpy permutation
(model.py:229-234), SGD lr = 0.7 (model.py:237), random.shuffle of the train list per epoch,
micro/macro F1 on the validation split (model.py:256-258), mean batch time (model.py:259).
Single process: the per-epoch shuffle is `random.shuffle(train)` on Python's GLOBAL stream, the one the strict
path's neighbour sampling also draws from -- as model.py:243 -- so a strict run consumes `random` call for
call like the reference.  Data parallel (world_size > 1): the shuffle draws from a generator of its OWN
(`random.Random(seed)`), because the samplers consume the global stream by a shard-dependent amount and ranks
sharing it would hold different permutations of `train`: `shard_batch` would slice overlapping / incomplete
shards.  With the private generator every rank holds the same permutation and the shards tile the global batch.
Deliberately different: batches are plain `batch_size` slices by default; `ref_batching=True`
reproduces the reference's `train[batch:max(train_num, batch+batch_size)]` descending batches
(model.py:244, a `max` where `min` was meant).  Everything stays on the GPU; with world_size > 1
each rank embeds its shard of the batch and the weight gradients are summed with one RCCL
all-reduce per step (dist.py).
"""
import random
import time

import numpy as np
import torch
import torch.nn as nn
from torch.nn import init

from . import dist
from .aggregators import MeanAggregator
from .encoders import Encoder
from .head import _sum_over_batch, head_grads, head_predict  # noqa: F401  (_sum_over_batch: its old home, still imported from here)
from .native import ACT_RELU, ACT_SIGMOID


class SupervisedGraphSage(nn.Module):
    """model.py:52-69."""

    def __init__(self, num_classes, enc):
        super(SupervisedGraphSage, self).__init__()
        self.enc = enc
        self.xent = nn.CrossEntropyLoss()
        self.weight = nn.Parameter(torch.FloatTensor(num_classes, enc.embed_dim))
        init.xavier_uniform_(self.weight)

    def forward(self, nodes):
        embeds = self.enc(nodes)
        scores = self.weight.to(embeds.device).mm(embeds)
        return scores.t()

    def loss(self, nodes, labels):
        scores = self.forward(nodes)
        return self.xent(scores, labels.squeeze().to(scores.device))


def build_model(feat_data, adj_lists, num_classes, hidden1=50, hidden2=128, num_sample1=10, num_sample2=10, gcn=True,
                cuda=True):
    """model.py:214-227 with this package's classes (num_sample defaults to 10/10: what the reference
    actually uses, its `enc.num_samples = ...` assignments being no-ops)."""
    n, d = feat_data.shape
    features = nn.Embedding(n, d)
    features.weight = nn.Parameter(torch.as_tensor(feat_data, dtype=torch.float32), requires_grad=False)
    agg1 = MeanAggregator(features, cuda=cuda)
    enc1 = Encoder(features, d, hidden1, adj_lists, agg1, num_sample=num_sample1, gcn=gcn, cuda=cuda)
    agg2 = MeanAggregator(lambda nodes: enc1(nodes).t(), cuda=cuda)
    enc2 = Encoder(lambda nodes: enc1(nodes).t(), enc1.embed_dim, hidden2, adj_lists, agg2, num_sample=num_sample2,
                   base_model=enc1, gcn=gcn, cuda=cuda)
    return SupervisedGraphSage(num_classes, enc2)


def run_training(feat_data, labels, adj_lists, num_classes, seed=1, epochs=1, batch_size=128, ref_batching=False, lr=0.7,
                 model=None, verbose=True, sample_seed=None, return_model=False, on_batch=None, **model_kwargs):
    """-> dict(f1_micro, f1_macro, mean_batch_time, losses).  Mirrors run_model (model.py:184-259).
    `seed` seeds numpy (the split) and Python's random (shuffles + neighbour sampling) as model.py:192-193
    does; `sample_seed` reseeds only Python's random, to vary the sampling stream on a fixed split.  With
    world_size > 1 the shuffles come from a private `random.Random(seed)` instead (module docstring)."""
    random.seed(seed if sample_seed is None else sample_seed)
    rank, world = (torch.distributed.get_rank(), dist.world_size()) if dist.world_size() > 1 else (0, 1)
    num_nodes = feat_data.shape[0]
    if model is None:
        model = build_model(feat_data, adj_lists, num_classes, **model_kwargs)
    params = [p for p in model.parameters() if p.requires_grad]
    dist.broadcast_params(params)
    test, val, train = _split(num_nodes, seed)
    train = list(train)
    optimizer = torch.optim.SGD(params, lr=lr)
    # world 1: the global stream, as model.py:243; world > 1: a generator identical on every rank, untouched by neighbour sampling
    shuffler = random if world == 1 else random.Random(seed)
    labels_t = torch.as_tensor(labels, dtype=torch.int64).squeeze(-1)
    times, losses = [], []
    for _ in range(epochs):
        shuffler.shuffle(train)
        for batch in range(0, len(train), batch_size):
            hi = max(len(train), batch + batch_size) if ref_batching else min(len(train), batch + batch_size)
            batch_nodes = train[batch:hi]
            mine = dist.shard_batch(batch_nodes, rank, world)
            if on_batch is not None:
                on_batch(batch_nodes, mine)       # test hook: which nodes this rank was given
            start = time.time()
            optimizer.zero_grad()
            if len(mine):
                scores = model(mine)
                tgt = labels_t[np.asarray(mine)].to(scores.device)
                # sum of per-sample losses / GLOBAL batch size: the all-reduce SUM is then the full-batch gradient
                loss = nn.functional.cross_entropy(scores, tgt, reduction="sum") / len(batch_nodes)
                loss.backward()
                losses.append(float(loss.detach()) * len(batch_nodes) / len(mine))
            dist.all_reduce_grads(params)
            optimizer.step()
            if torch.cuda.is_available():
                torch.cuda.synchronize()
            times.append(time.time() - start)
    with torch.no_grad():
        val_output = model(val)
    micro, macro = _f1(labels, val, val_output.detach().cpu().numpy().argmax(axis=1))
    res = {"f1_micro": micro, "f1_macro": macro,
           "mean_batch_time": float(np.mean(times)) if times else 0.0, "losses": losses, "test_nodes": test}
    if return_model:
        res["model"] = model
    if verbose and rank == 0:
        print("Validation F1 micro:", res["f1_micro"])
        print("Validation F1 macro:", res["f1_macro"])
        print("Average batch time:", res["mean_batch_time"])
    return res


def _split(n, seed):
    """(test, val, train): numpy's global generator seeded with `seed`, the 10 / 10 / 80 split of its permutation of n (model.py:192, 229-234)."""
    np.random.seed(seed)
    rand_indices = np.random.permutation(n)
    return rand_indices[:int(0.1 * n)], rand_indices[int(0.1 * n):int(0.2 * n)], rand_indices[int(0.2 * n):]


def _f1(labels, val, pred):
    """(micro, macro) F1 of the predictions `pred` for the nodes `val` (model.py:256-258)."""
    from sklearn.metrics import f1_score
    truth = np.asarray(labels)[val].reshape(-1)
    return float(f1_score(truth, pred, average="micro")), float(f1_score(truth, pred, average="macro"))


def _batches(train, shuffler, epochs, batch_size, ref_batching, dev):
    """The mini-batches of `epochs` epochs as contiguous int32 device tensors of node ids: `train` (a list, shuffled in place by
    shuffler.shuffle at the start of every epoch and uploaded once per epoch) in batch_size slices, or with ref_batching in the
    reference's descending `train[batch:max(train_num, batch + batch_size)]` (module docstring)."""
    for _ in range(epochs):
        shuffler.shuffle(train)
        order = torch.as_tensor(np.asarray(train), dtype=torch.int32).to(dev)
        for lo in range(0, len(train), batch_size):
            hi = max(len(train), lo + batch_size) if ref_batching else min(len(train), lo + batch_size)
            yield order[lo:hi].contiguous()


def _validation_result(labels, val, pred, elapsed, steps, losses, trainer):
    """What the run drivers of the three trainers return: dict(f1_micro, f1_macro, mean_step_time, losses, trainer); pred: the
    trainer's classes of the validation nodes `val`, on the device."""
    micro, macro = _f1(labels, val, pred.cpu().numpy())
    return {"f1_micro": micro, "f1_macro": macro, "mean_step_time": elapsed / max(steps, 1), "losses": [float(x) for x in losses],
            "trainer": trainer}


def check_trainer_args(who, head, act1, hidden2, num_classes, table=None, embed_index=None, embed_rows=None, embed_dim=None):
    """The refusals the three trainers share, in the name of the class `who`: the head, layer 1's activation, a table AND an index, an
    index without the embedding's shape, a native head without a kernel for the shape.  A trainer passes what it has."""
    from . import native, ops
    if head not in ("torch", "native"):
        raise native.SageError(f"{who}: head = {head!r}, expected 'torch' or 'native'")
    if act1 not in (ACT_RELU, ACT_SIGMOID):
        raise native.SageError(f"{who}: act1 = {act1!r}, expected ACT_RELU or ACT_SIGMOID")
    if embed_index is not None:
        ops.refuse_bf16(table, f"{who}(embed_index=)")
    if embed_index is not None and table is not None:
        raise native.SageError(f"{who}: table and embed_index are alternatives: layer 1 reads one of them")
    if embed_index is not None and (embed_rows is None or embed_dim is None or int(embed_rows) < 1 or int(embed_dim) < 1):
        raise native.SageError(f"{who}: embed_rows = {embed_rows!r}, embed_dim = {embed_dim!r}")
    if head == "native" and not ops.xent_head_supported(hidden2, num_classes):
        raise native.SageError(f"{who}: head='native' has no kernel for hidden2 = {hidden2}, num_classes = {num_classes}")


def init_parameters(dev, d0, hidden1, hidden2, num_classes, gcn, embed_rows=None):
    """(w1, w2, w_cls, embed | None) on `dev`, drawn in this order from torch's generator -- one torch seed gives every trainer the same
    start: the three weights xavier_uniform_ (encoders.py:36-38, model.py:61-62), then, with embed_rows, the embedding
    [embed_rows, d0] N(0, 1) as nn.Embedding's weight is (aggregators.py:31) -- AFTER the three weights, which therefore start as a
    frozen-table trainer's do.  The caller broadcasts them (dist.broadcast_params)."""
    m = 1 if gcn else 2
    w1 = torch.empty(hidden1, m * d0, device=dev)
    w2 = torch.empty(hidden2, m * hidden1, device=dev)
    w_cls = torch.empty(num_classes, hidden2, device=dev)
    for w in (w1, w2, w_cls):
        init.xavier_uniform_(w)
    embed = None
    if embed_rows is not None:
        embed = torch.empty(int(embed_rows), d0, device=dev)
        init.normal_(embed)
    return w1, w2, w_cls, embed


def csr_pair(rowptr, col, rowptr_outer=None, col_outer=None):
    """The layer-1 CSR checked and the layer-2 CSR (default: the same) -> (rowptr_outer, col_outer), as FullGraphTrainer and
    ExactBatchTrainer take them."""
    from . import native, ops
    ops._chk(rowptr, torch.int64, "rowptr", 1)
    ops._chk(col, torch.int32, "col", 1)
    rowptr2 = rowptr if rowptr_outer is None else ops._chk(rowptr_outer, torch.int64, "rowptr_outer", 1)
    col2 = col if col_outer is None else ops._chk(col_outer, torch.int32, "col_outer", 1)
    if rowptr2.shape[0] != rowptr.shape[0]:
        raise native.SageError("inner and outer CSR must cover the same node ids")
    return rowptr2, col2


class EngineTrainer:
    """One SGD step of SupervisedGraphSage (model.py:52-69, 240-252: forward, CrossEntropy, backward, SGD lr 0.7) with NOTHING
    on the host but enqueues: device sampler at both hops and both layers through TwoHopEngine (sage_forward2), the classifier and
    the loss as a handful of torch ops on the same stream, the backward through the engine's own intermediates (nbr / cnt / row2 / h1
    stay in its workspace) with the C-ABI backward kernels, and in-place SGD updates.  No host synchronisation inside a step: the
    frontier size never leaves the device (every kernel takes its row count from the workspace).  run_training above is the
    module-level path (the reference's class surface: since round 3 it runs the same engine forward and backward as ONE autograd
    node, ~1.2 ms per 256-seed step with the host-side classifier of model.py); this is the throughput path: 0.42 ms per 256-seed
    step on stand-in Cora (0.24 ms as a captured hipGraph), 0.31 ms per 4096-seed step at config-3 size, against 140-180 ms for
    the reference on a CPU.

    table is frozen (model.py:214-215), so layer 1 needs no input gradient.  Gradients follow torch autograd of the reference's
    expression: d relu, d sigmoid, d mean = 1/|set| per member -- TwoHopEngine.backward_weights: sage_linear_act_backward_ws for
    layer 2, sage_two_hop_grad_w1 (the layer-1 weight gradient summed over the outer samples) for layer 1; no float atomics, two
    runs of one schedule give the same bits.

    Featureless graphs (aggregators.py:68-71, --initializer 1hot / node_degree): table=None with embed_index int32 [N] (values in
    [0, embed_rows)), embed_rows and embed_dim -- FullGraphTrainer's argument names and rules.  Layer 1 then reads the trainable
    self.embed_weight [embed_rows, embed_dim] (drawn N(0, 1) as nn.Embedding's weight is, AFTER the three weights, which therefore start
    as the frozen trainer's do for the same torch seed) through the index: the engine samples embedding rows (TwoHopEngine's
    embed_index), parameters() and grads() gain a fourth entry, step() updates the embedding in place with the dense [embed_rows,
    embed_dim] gradient of backward_weights(need_embed=True).  gcn encoder without the aggregator's self loop, no relabel,
    embed_dim % 4 == 0; no captured step and no data-parallel step in this form.  act1: layer 1's activation (node_degree uses
    sigmoid, encoders.py:58-59).
    sparse_embed=True (an embedding trainer only; the default stays False): step() applies the embedding's update to the rows the batch
    touched and to nothing else, inside the gradient call itself (backward_weights(need_embed="update"): embed[e] = fma(-lr, g[e],
    embed[e]), one rounding), and grads() returns the compact triple (rows, num_rows, grad_rows) -- buffers of the engine, rewritten by
    the next call -- as its fourth entry: no [embed_rows, embed_dim] tensor exists anywhere in the step.  For a 1hot table of millions
    of rows; a small table (node_degree) gains little."""

    def __init__(self, rowptr, col, table, num_classes, hidden1=50, hidden2=128, num_sample1=10, num_sample2=10, gcn=True, lr=0.7,
                 max_batch=256, agg_self_loop=False, relabel=None, head="torch", embed_index=None, embed_rows=None, embed_dim=None,
                 act1=ACT_RELU, sparse_embed=False):
        """head: "torch" -- the classifier, its loss and their gradients as stock torch ops (the default: its bits are the recorded
        w_cls trajectories); "native" -- one sage_xent_head call, its sums in an order fixed by the shape.  With the
        native head the loss and the classifier gradient that grads() returns live in buffers of the trainer, rewritten by its next call."""
        from . import native, ops
        check_trainer_args("EngineTrainer", head, act1, hidden2, num_classes, table, embed_index, embed_rows, embed_dim)
        ops.refuse_bf16(table, "EngineTrainer")
        if sparse_embed and embed_index is None:
            raise native.SageError("EngineTrainer: sparse_embed needs embed_index: a frozen table has no update to make sparse")
        if embed_index is not None and dist.world_size() > 1:
            raise native.SageError("EngineTrainer: a trainable embedding is single-process in this build (its gradient is not all-reduced)")
        self.head = head
        from .engine import TwoHopEngine
        dev = table.device if embed_index is None else embed_index.device
        d0 = table.shape[1] if embed_index is None else int(embed_dim)
        self.w1, self.w2, self.w_cls, self.embed_weight = init_parameters(dev, d0, hidden1, hidden2, num_classes, gcn,
                                                                          None if embed_index is None else embed_rows)
        self.lr = float(lr)
        self.sparse_embed = bool(sparse_embed)
        self.concat = not gcn
        # data parallel: every rank starts from rank 0's weights.  BEFORE the engine is built: its constructor prepares the bf16
        # planes of W1 (and zero-padded copies of odd widths) and caches them under (data_ptr, _version), which a broadcast
        # through `.data` does not move -- ranks != 0 would run their first step on planes of their own initial W1
        dist.broadcast_params(self.parameters())
        self.engine = TwoHopEngine(rowptr, col, table if embed_index is None else self.embed_weight, self.w1, self.w2, num_sample1,
                                   num_sample2, concat=self.concat, agg_self_loop=agg_self_loop, act1=act1, max_batch=max_batch,
                                   relabel=relabel, embed_index=embed_index)
        self.engine.keep_means = True        # the backward reads the layer-1 means of the forward from the workspace
        self.engine.invalidate_weights()
        self._native, self._ops = native, ops
        # the caller's graph and table (the engine may work on renumbered copies): what embed_exact reads
        self._exact = {"rowptr": rowptr, "col": col, "table": table, "index": embed_index, "frontier": None}
        self._out_q = None
        self._step_graph = None
        self._head = None
        if head == "native":
            self._head_reserve(max_batch)

    def _head_reserve(self, rows):
        """Outputs and workspace of the native head for batches of up to `rows` seeds: allocated here, never inside a (captured) step."""
        c, h2 = self.w_cls.shape
        dev = self.w_cls.device
        self._head = {"rows": int(rows), "loss": torch.zeros(1, device=dev), "grad_emb": torch.empty(rows, h2, device=dev),
                      "grad_w": torch.empty(c, h2, device=dev), "pred": torch.empty(rows, dtype=torch.int32, device=dev),
                      "workspace": torch.empty(self._ops.xent_head_workspace_bytes(rows, h2, c), dtype=torch.uint8, device=dev)}

    def parameters(self):
        return [self.w1, self.w2, self.w_cls] + ([] if self.embed_weight is None else [self.embed_weight])

    def _backward(self, out, g_out, embed_lr=None):
        """The engine's gradients behind the classifier's: (g_w1, g_w2), and the embedding's where there is one: dense, or on a sparse
        trainer the compact triple -- with embed_lr the update is applied instead and the third entry is the touched-row count."""
        if self.sparse_embed:
            return self.engine.backward_weights(out, g_out, need_embed="rows" if embed_lr is None else "update", embed_lr=embed_lr)
        return self.engine.backward_weights(out, g_out, need_embed=self.embed_weight is not None)

    def embed(self, seeds, key=0):
        """[B, hidden2] embeddings (no grad): the evaluation forward."""
        return self.engine.forward(seeds, seed=key)

    def scores(self, seeds, key=0):
        return self.embed(seeds, key) @ self.w_cls.t()

    def predict(self, seeds, key=0):
        """int32 [B]: the class of the highest score of one sampled forward (head.head_predict: model.py:256)."""
        return self._predict_of(self.embed(seeds, key))

    def _predict_of(self, emb):
        """predict()'s rule on given embeddings; the native head works in the trainer's reserved buffers."""
        if self.head != "native":
            return head_predict(emb, self.w_cls, self.head)
        if emb.shape[0] > self._head["rows"]:
            self._head_reserve(emb.shape[0])
        hd = self._head
        return head_predict(emb, self.w_cls, self.head, workspace=hd["workspace"], out={"pred": hd["pred"]}).clone()

    def embed_exact(self, seeds):
        """[B, hidden2] embeddings over the FULL neighbourhoods at both hops (aggregators.py:47-48, num_sample=None): no sampler key, the
        same bits on every call -- inference.embed_nodes on the trainer's own weights and its table (the embedding through embed_index
        on an embedding trainer), in the caller's node ids.  The [N] frontier map is built at the first call and kept; two host reads
        per call (embed_nodes)."""
        from .inference import embed_nodes
        ex, eng = self._exact, self.engine
        if ex["frontier"] is None:
            ex["frontier"] = self._ops.CsrFrontier(ex["rowptr"].shape[0] - 1, self.w1.device, max_nodes=0)
        with torch.no_grad():
            return embed_nodes(ex["rowptr"], ex["col"], ex["table"] if ex["index"] is None else self.embed_weight, self.w1, self.w2, seeds,
                               concat=self.concat, agg_self_loop=eng.agg_self_loop, act1=eng.act1, act2=eng.act2, nan_empty=eng.nan_empty,
                               index=ex["index"], frontier=ex["frontier"])

    def predict_exact(self, seeds):
        """predict() on embed_exact's embeddings: int32 [B], identical on every call."""
        return self._predict_of(self.embed_exact(seeds))

    def grads(self, seeds, labels, key, global_batch=None, _embed_lr=None):
        """loss (device scalar) and the gradients of (w1, w2, w_cls) -- and of embed_weight, a fourth entry, on an embedding trainer
        (dense [embed_rows, embed_dim]; with sparse_embed the triple (rows, num_rows, grad_rows) of the touched rows) -- for one batch;
        nothing is updated (_embed_lr is step()'s: on a sparse trainer the embedding's update is applied inside the gradient call and
        the fourth entry is the touched-row count).
        global_batch: data parallel -- this rank holds a shard of a mini-batch of that many seeds; its loss is the SUM over its
        shard / global_batch, so that the SUM of the ranks' gradients is the full-batch gradient."""
        e = self.engine
        if seeds is None:                                                  # the batch at the engine's queue cursor (capturable step)
            b = e._queue_batch
            if self._out_q is None or self._out_q.shape[0] != b:
                self._out_q = torch.empty(b, e.h2, device=e.device)
            out = e.forward_queued(self._out_q)
        else:
            b = seeds.shape[0]
            out = e.forward(seeds, seed=key)                               # sample, frontier, sample, layer 1, layer 2
        hd = {}
        if self.head == "native":                                          # the head works in the trainer's buffers: no allocation in a step
            if b > self._head["rows"]:
                self._head_reserve(b)                                      # never while capturing: capture_step's batch is <= max_batch
            hd = dict(workspace=self._head["workspace"], out=self._head)
        # classifier + loss + their gradients on the same stream (model.py:59-69)
        loss, g_out, g_cls = head_grads(out, self.w_cls, labels, self.head, b, global_batch, **hd)
        # both layers' weight gradients from the intermediates this forward left in the engine's workspace
        g_w1, g_w2, *g_e = self._backward(out, g_out, _embed_lr)
        if self.head == "native" and seeds is not None:
            # the loss lives in the trainer's buffer.  Eager: the caller may keep the loss of every step (run_engine_training does);
            # queued: the captured step copies it at once
            loss = loss.clone()
        return loss, (g_w1, g_w2, g_cls, *g_e)

    def step(self, seeds, labels, key, global_batch=None):
        """forward + backward + SGD; -> loss as a device scalar (reading it is the caller's only synchronisation).
        With torch.distributed initialised (one process per GPU, backend "nccl" = RCCL over xGMI) the three weight gradients
        travel in ONE flat all-reduce (SUM) per step, ~0.3 MB: latency bound, so one buffer and one call."""
        loss, (g1, g2, gc, *ge) = self.grads(seeds, labels, key, global_batch, _embed_lr=self.lr if self.sparse_embed else None)
        if ge and not self.sparse_embed:                      # (sparse: the touched rows were updated inside the gradient call)
            self.embed_weight.add_(ge[0], alpha=-self.lr)     # in place: the engine reads this very tensor at the next forward
        if dist.world_size() > 1:
            flat = torch.cat([g1.reshape(-1), g2.reshape(-1), gc.reshape(-1)])
            torch.distributed.all_reduce(flat, op=torch.distributed.ReduceOp.SUM)
            n1, n2 = g1.numel(), g2.numel()
            g1, g2, gc = flat[:n1].view_as(g1), flat[n1:n1 + n2].view_as(g2), flat[n1 + n2:].view_as(gc)
        self.w1.add_(g1, alpha=-self.lr)
        self.w2.add_(g2, alpha=-self.lr)
        self.w_cls.add_(gc, alpha=-self.lr)
        return loss


    # ---- the whole step as ONE hipGraph ("graph-capturable fwd+bwd") ------------------------------------------------
    def capture_step(self, seeds_ring, keys, labels_by_node):
        """seeds_ring: int32 device tensor [S, B] of mini-batches, keys: S sampler keys, labels_by_node: int64 device tensor [N].
        Captures forward + loss + backward + SGD of the batch at the engine's queue cursor into one torch.cuda.CUDAGraph:
        replay_step() then trains on batch after batch of the ring (wrapping around) with a single graph launch each, nothing
        read from the host: the seeds and the sampler key come from the device-side ring (sage_batch_t), the labels are
        gathered by the ids at the cursor, the weight planes are re-prepared inside the graph after every update.
        -> the static device scalar that holds the last replayed step's loss."""
        e = self.engine
        if self.embed_weight is not None:
            raise self._native.SageError("capture_step: not provided for a trainable embedding in this build (its gradient chain allocates "
                                         "scratch on first use and has not been captured)")
        if dist.world_size() > 1:
            raise self._native.SageError("capture_step: single-process only (the data-parallel step has a collective per step)")
        e.set_queue(seeds_ring, keys)
        ring, nring = e._queue_seeds, seeds_ring.shape[0]
        labels_by_node = labels_by_node.to(e.device)
        self._loss_static = torch.zeros((), device=e.device)

        def one():
            cur = torch.remainder(e._cursor.to(torch.int64), nring)       # read BEFORE the forward's last kernel advances the cursor
            ids = ring.index_select(0, cur)[0]
            labels = labels_by_node.index_select(0, ids.to(torch.int64))
            self._loss_static.copy_(self.step(None, labels, None))

        saved = [w.clone() for w in self.parameters()]
        side = torch.cuda.Stream(device=e.device)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):                                     # warm-up outside capture: a real step, undone below
            one()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            one()
        with torch.no_grad():
            for w, w0 in zip(self.parameters(), saved):
                w.copy_(w0)
        e._model()                                                        # planes of the restored W1
        e.rewind(0)
        torch.cuda.synchronize()
        self._step_graph = g
        return self._loss_static

    def replay_step(self):
        self._step_graph.replay()
        # the replay updated the weights without moving their version counters: an eager forward after it (validation, a
        # plain step) must not find its cached planes / padded copies of W_{t-1} "up to date" 
        self.engine.invalidate_weights()
        return self._loss_static


def run_engine_training(graph, feat_data, labels, num_classes, seed=1, epochs=1, batch_size=128, ref_batching=False, lr=0.7,
                        sample_seed=0, hidden1=50, hidden2=128, num_sample1=10, num_sample2=10, gcn=True, head="torch", initializer=None,
                        embed_dim=100, sparse_embed=False, exact_eval=False, act1=None):
    """run_model (model.py:184-259) on the engine path: same split, shuffles, batching and optimiser as run_training above, every
    step through EngineTrainer.  -> dict(f1_micro, f1_macro, mean_step_time, losses, trainer).
    initializer: None (or "None") -- the frozen table feat_data; "1hot" -- a trainable embedding row per node, ReLU; "node_degree" -- a
    row per degree, SIGMOID at layer 1 (encoders.py:58-59).  feat_data is not read for the last two and may be None; embed_dim is
    the embedding's width (the reference's --feature_dim default), a multiple of 4.  sparse_embed: EngineTrainer's (an initializer
    only): update the touched embedding rows alone.  exact_eval: the validation predictions come from predict_exact (full
    neighbourhoods, no sampler key) instead of one sampled forward; training is the same either way.  act1: layer 1's activation over
    the frozen table (None: ReLU), ACT_SIGMOID for datasets.pagerank_table; refused with an initializer, which sets its own."""
    from .fullgraph import embed_arguments, frozen_arguments
    dev = torch.device("cuda")
    embed = embed_arguments("run_engine_training", initializer, (None, "None"), graph, embed_dim, dev, act1)
    rowptr, col = graph.to(dev)
    table = torch.as_tensor(feat_data, dtype=torch.float32).to(dev) if embed is None else None
    _, val, train = _split(graph.num_nodes, seed)
    train = list(train)
    top = len(train) if ref_batching else batch_size
    tr = EngineTrainer(rowptr, col, table, num_classes, hidden1, hidden2, num_sample1, num_sample2, gcn=gcn, lr=lr, max_batch=max(top, len(val)),
                       head=head, sparse_embed=sparse_embed, **(embed or frozen_arguments(act1)))
    labels_dev = torch.as_tensor(np.asarray(labels).reshape(-1), dtype=torch.int64).to(dev)
    losses, key = [], int(sample_seed) << 20
    torch.cuda.synchronize()
    t0 = time.time()
    for ids in _batches(train, random.Random(seed), epochs, batch_size, ref_batching, dev):
        losses.append(tr.step(ids, labels_dev[ids.long()], key))
        key += 1
    torch.cuda.synchronize()
    elapsed = time.time() - t0
    with torch.no_grad():
        val_ids = torch.as_tensor(val.astype(np.int32)).to(dev)
        pred = tr.predict_exact(val_ids) if exact_eval else tr.predict(val_ids, key=key)
    return _validation_result(labels, val, pred, elapsed, len(losses), losses, tr)
