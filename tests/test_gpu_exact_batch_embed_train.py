"""Exact mini-batch training of node and degree embeddings (sage355.exactbatch.ExactBatchEmbedTrainer): the 1hot / node_degree
initializers on full neighbourhoods of a seed batch, the embedding's gradient through sage_csr_mean_backward_rows (dense) or
sage_csr_mean_backward_touched (sparse_embed: touched rows only, the SGD update fused in).  The setup is
tests/test_gpu_exact_batch_train.py's: the start and the forward bit for bit against the whole-graph trainer and embed_nodes, loss and
the classifier's gradient bit for bit against the whole-graph trainer, the gradients of w1, w2 and the embedding against fp64 torch
autograd of the dense expression at tests/test_gpu_fullgraph_embedding.py's bars for that expression (max |g - ref| / max|ref| <=
2e-5, loss 1e-5), the sparse form against the dense one, run-to-run bit identity, the state of the id -> row map, memory that follows
the batch and not the table, and that training lowers the loss."""
import os

import numpy as np
import pytest
import torch

from sage355 import native
from sage355.datasets import standin_citation
from sage355.exactbatch import ExactBatchEmbedTrainer, run_exact_batch_training
from sage355.fullgraph import FullGraphTrainer, degree_index, one_hot_index
from sage355.graph import CSRGraph, rmat_graph
from sage355.inference import embed_nodes
from sage355.native import ACT_RELU, ACT_SIGMOID
from util import GOLDEN_DIR

pytestmark = pytest.mark.gpu
DEV = "cuda"
CLASSES, TRAIN = 5, 300
U32 = 2.0 ** -24


def bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.fixture(scope="module")
def setup():
    graph = rmat_graph(11, 30_000, seed=4, accel=None)                 # 2048 nodes, a hub of 768 entries, 333 isolated nodes
    deg = graph.degrees()
    n = graph.num_nodes
    assert n == 2048 and int(deg.max()) > native.CSR_MEAN_CHUNK and int((deg == 0).sum()) > 0
    rs = np.random.default_rng(2)
    ids = rs.choice(n, TRAIN, replace=False)                          # distinct; isolated nodes and the hub's neighbours among them
    labels = torch.from_numpy(rs.integers(0, CLASSES, TRAIN))
    rowptr, col = graph.to(DEV)
    indices = {"1hot": one_hot_index(n, DEV) + (ACT_RELU,), "node_degree": degree_index(rowptr) + (ACT_SIGMOID,)}
    # the batch's structure, on the host: the frontier, and the embedding rows its inner terms go to
    frontier = np.unique(np.concatenate([ids] + [graph.col[graph.rowptr[v]:graph.rowptr[v + 1]] for v in ids]))
    inner = np.concatenate([graph.col[graph.rowptr[v]:graph.rowptr[v + 1]] for v in frontier])
    print(f"frontier {len(frontier)} nodes, {len(inner)} inner terms")
    for name, (index, rows, _) in indices.items():
        runs = np.bincount(index.cpu().numpy()[inner], minlength=rows)
        print(f"{name}: {rows} rows, {int((runs > 0).sum())} touched, longest run {int(runs.max())}, {int((runs > native.CSR_MEAN_CHUNK).sum())} "
              f"runs of more than one chunk")
        assert runs.max() > native.CSR_MEAN_CHUNK and (runs == 0).any(), f"{name}: a run of more than one chunk and an untouched row"
    src = torch.from_numpy(np.repeat(np.arange(n), np.diff(graph.rowptr)))
    dst = torch.from_numpy(graph.col.astype(np.int64))
    own = np.zeros(n, dtype=bool)
    own[src[dst == src].numpy()] = True
    return dict(graph=graph, rowptr=rowptr, col=col, ids=ids, labels=labels, indices=indices, src=src, dst=dst, own=own, deg=deg,
                seeds=torch.from_numpy(ids.astype(np.int32)).to(DEV), tgt=labels.to(DEV))


def _trainer(s, initializer, seed=3, **kw):
    index, rows, act1 = s["indices"][initializer]
    torch.manual_seed(seed)
    return ExactBatchEmbedTrainer(s["rowptr"], s["col"], CLASSES, index, rows, kw.pop("embed_dim", 64), act1=act1, **kw)


def _autograd_reference(s, tr):
    """fp64 torch autograd of the dense expression: X = embed[index], mean by index_add over the edges (zeros for an empty set, the
    set-union self term with self_loop), concat, W.x, the layer's activation, classifier, cross_entropy on the training rows."""
    n = s["graph"].num_nodes
    extra = torch.from_numpy((~s["own"]) if tr.self_loop else np.zeros(n, dtype=bool)).double()
    cnt = torch.from_numpy(s["deg"].astype(np.float64)) + extra
    inv = torch.where(cnt > 0, 1.0 / cnt.clamp_min(1.0), torch.zeros_like(cnt))

    def mean(x):
        return (torch.zeros_like(x).index_add(0, s["src"], x[s["dst"]]) + x * extra[:, None]) * inv[:, None]

    w1, w2, wc, emb = (w.detach().cpu().double().requires_grad_(True) for w in tr.parameters())
    x = emb[tr.embed_index.cpu().long()]
    agg1 = mean(x)
    pre1 = (torch.cat([x, agg1], 1) if tr.concat else agg1) @ w1.t()
    h1 = torch.sigmoid(pre1) if tr.act1 == ACT_SIGMOID else torch.relu(pre1)
    agg2 = mean(h1)
    out = torch.relu((torch.cat([h1, agg2], 1) if tr.concat else agg2) @ w2.t())
    loss = torch.nn.functional.cross_entropy(out[torch.from_numpy(s["ids"])] @ wc.t(), s["labels"])
    return loss.item(), torch.autograd.grad(loss, (w1, w2, wc, emb))


@pytest.mark.parametrize("head", ["native", "torch"])
@pytest.mark.parametrize("embed_dim,h1", [(64, 32), (50, 30)])
@pytest.mark.parametrize("self_loop", [False, True])
@pytest.mark.parametrize("gcn", [True, False])
@pytest.mark.parametrize("initializer", ["1hot", "node_degree"])
def test_exact_batch_embedding_forward_loss_and_gradients(setup, initializer, gcn, self_loop, embed_dim, h1, head):
    s = setup
    index, rows, act1 = s["indices"][initializer]
    kw = dict(hidden1=h1, hidden2=64, gcn=gcn, agg_self_loop=self_loop, head=head)
    tr = _trainer(s, initializer, embed_dim=embed_dim, **kw)
    torch.manual_seed(3)
    full = FullGraphTrainer(s["rowptr"], s["col"], None, CLASSES, embed_index=index, embed_rows=rows, embed_dim=embed_dim, act1=act1, **kw)
    assert len(tr.parameters()) == 4 and tr.parameters()[3] is tr.embed and tuple(tr.embed.shape) == (rows, embed_dim)
    for a, b in zip(tr.parameters(), full.parameters()):
        assert bits_equal(a, b), "one torch seed must give both trainers the same start"
    # the forward: embed_nodes' bits through the index, and the whole-graph trainer's
    got = tr.forward(s["seeds"])
    assert not bool(torch.isnan(got).any())
    assert bits_equal(got, embed_nodes(s["rowptr"], s["col"], tr.embed, tr.w1, tr.w2, s["seeds"], concat=not gcn, agg_self_loop=self_loop,
                                       act1=act1, nan_empty=False, index=index))
    assert bits_equal(got, full.forward()[s["seeds"].long()]), "forward(seeds) differs from FullGraphTrainer.forward()[seeds]"
    # the head sees the same rows in the same order: loss and dW_cls bit for bit
    loss, grads = tr.grads(s["seeds"], s["tgt"])
    full_loss, full_grads = full.grads(s["seeds"], s["tgt"])
    assert len(grads) == 4 and grads[3].shape == tr.embed.shape
    assert bits_equal(loss.reshape(1), full_loss.reshape(1)), (loss.item(), full_loss.item())
    assert bits_equal(grads[2], full_grads[2]), "the gradient of w_cls differs from the whole-graph trainer's"
    assert bool((tr.frontier.pos == -1).all()), "the map is not clear after grads()"
    # all four against fp64
    ref_loss, ref = _autograd_reference(s, tr)
    print(f"loss {loss.item():.8f} ref {ref_loss:.8f}")
    errs = {}
    for name, g, r in zip(("w1", "w2", "w_cls", "embed"), grads, ref):
        errs[name] = (g.cpu().double() - r).abs().max().item() / r.abs().max().item()
    print("max |g - ref| / max|ref|:", {k: f"{v:.2e}" for k, v in errs.items()})
    assert abs(loss.item() - ref_loss) <= 1e-5 * max(1.0, abs(ref_loss))
    for name, err in errs.items():
        assert err <= 2e-5, f"grad {name}: max |g - ref| / max|ref| = {err:.2e}"
    untouched = (ref[3] == 0).all(1)
    assert bool(untouched.any()) and not bool(grads[3].cpu()[untouched].any()), "an embedding row the batch does not read must get exact zeros"


def fp64_update_check(new, old, g, lr, what):
    """|new - (old - lr g)| <= 2^-24 |old - lr g| (1 + 2^-20): one fp32 rounding of the exact value; the last factor covers the fp64
    reference's own rounding.  lr is the float32 the kernel is handed.  (tests/test_gpu_embed_sparse.py's check.)"""
    lr32 = float(np.float32(lr))
    ref = old.double() - lr32 * g.double()
    err = (new.double() - ref).abs()
    bound = U32 * ref.abs() * (1 + 2.0 ** -20)
    worst = float((err / bound.clamp_min(1e-300)).max())
    print(f"{what}: max |new - ref| = {float(err.max()):.3e}, max err / bound = {worst:.3f}")
    assert bool((err <= bound).all()), f"{what}: more than one rounding away from old - lr * g (ratio {worst:.3f})"


@pytest.mark.parametrize("head", ["native", "torch"])
@pytest.mark.parametrize("embed_dim,h1", [(64, 32), (50, 30)])
@pytest.mark.parametrize("self_loop", [False, True])
@pytest.mark.parametrize("initializer", ["1hot", "node_degree"])
def test_sparse_embed_is_the_dense_gradient_on_the_touched_rows(setup, initializer, self_loop, embed_dim, h1, head):
    s = setup
    kw = dict(embed_dim=embed_dim, hidden1=h1, hidden2=64, agg_self_loop=self_loop, head=head, lr=0.7)
    dense, sparse = _trainer(s, initializer, **kw), _trainer(s, initializer, sparse_embed=True, **kw)
    for a, b in zip(dense.parameters(), sparse.parameters()):
        assert bits_equal(a, b)
    loss_d, g_d = dense.grads(s["seeds"], s["tgt"])
    loss_s, g_s = sparse.grads(s["seeds"], s["tgt"])
    assert bits_equal(loss_d.reshape(1), loss_s.reshape(1))
    for a, b in zip(g_d[:3], g_s[:3]):
        assert bits_equal(a, b)
    rows, num, grad_rows = g_s[3]
    nu = int(num)
    idx = rows[:nu].long()
    assert 0 < nu < dense.embed.shape[0] and bool((idx[1:] > idx[:-1]).all())
    assert bits_equal(grad_rows[:nu], g_d[3][idx]), "grad_rows differs from the dense gradient's rows"
    rest = torch.ones(dense.embed.shape[0], dtype=torch.bool, device=DEV)
    rest[idx] = False
    assert bool((g_d[3][rest].view(torch.int32) == 0).all()), "the dense gradient is not exact zeros outside the touched rows"
    assert bits_equal(sparse.embed, dense.embed), "grads() must update nothing"
    # one step: the three weights as the dense trainer's, the touched rows one rounding from old - lr g, the others untouched
    old = sparse.embed.clone()
    l_d, l_s = dense.step(s["seeds"], s["tgt"]), sparse.step(s["seeds"], s["tgt"])
    assert bits_equal(l_d.reshape(1), l_s.reshape(1))
    for name, a, b in zip(("w1", "w2", "w_cls"), dense.parameters(), sparse.parameters()):
        assert bits_equal(a, b), f"{name} differs between the dense and the sparse step"
    fp64_update_check(sparse.embed[idx], old[idx], grad_rows[:nu], sparse.lr, f"{initializer} self_loop={self_loop} dim={embed_dim}")
    assert bits_equal(sparse.embed[rest], old[rest]), "a row the batch does not read was written"
    assert not bits_equal(sparse.embed[idx], old[idx]), "the embedding has not moved"
    assert bool((sparse.frontier.pos == -1).all())


@pytest.mark.parametrize("initializer,gcn,head,sparse", [("1hot", True, "native", False), ("node_degree", False, "torch", False),
                                                         ("1hot", False, "native", False), ("1hot", True, "torch", True),
                                                         ("node_degree", True, "native", True)])
def test_exact_batch_embedding_training_is_reproducible_bit_for_bit(setup, initializer, gcn, head, sparse):
    runs = []
    for _ in range(2):
        tr = _trainer(setup, initializer, seed=9, hidden1=32, hidden2=64, gcn=gcn, lr=0.3, agg_self_loop=True, head=head, sparse_embed=sparse)
        first = tr.embed.clone()
        losses = [tr.step(setup["seeds"], setup["tgt"]).clone() for _ in range(5)]
        assert not bits_equal(first, tr.embed), "the embedding has not moved"
        runs.append((torch.stack(losses), [w.clone() for w in tr.parameters()]))
    (la, wa), (lb, wb) = runs
    assert bits_equal(la, lb), (la.tolist(), lb.tolist())
    assert len(wa) == 4
    for name, a, b in zip(("w1", "w2", "w_cls", "embed"), wa, wb):
        assert bits_equal(a, b), f"{name}: two runs differ at {int((a != b).sum())} elements"
    assert bool(torch.isfinite(la).all())


@pytest.mark.parametrize("sparse", [False, True])
def test_the_map_is_clear_after_a_step_and_after_a_step_that_raised(setup, sparse):
    s = setup
    tr = _trainer(s, "node_degree", hidden1=32, hidden2=64, gcn=sparse, sparse_embed=sparse)
    seeds, tgt = s["seeds"], s["tgt"]
    tr.step(seeds, tgt)
    assert bool((tr.frontier.pos == -1).all()) and int(tr.frontier.count) == 0
    bad = seeds.clone()
    bad[17] = s["graph"].num_nodes + 4
    with pytest.raises(native.SageError):
        tr.step(bad, tgt)
    assert bool((tr.frontier.pos == -1).all()) and int(tr.frontier.count) == 0
    with pytest.raises(native.SageError):                              # labels of another length
        tr.grads(seeds, tgt[:-1])
    assert bool((tr.frontier.pos == -1).all())
    before = tr.embed.clone()
    loss = tr.step(seeds, tgt)                                         # and the trainer still works, and predict reads the new embedding
    assert bool(torch.isfinite(loss)) and not bits_equal(before, tr.embed)
    pred = tr.predict(seeds)
    assert pred.dtype == torch.int32 and pred.shape == seeds.shape and int(pred.min()) >= 0 and int(pred.max()) < CLASSES
    assert bits_equal(tr.forward(seeds), embed_nodes(s["rowptr"], s["col"], tr.embed, tr.w1, tr.w2, seeds, concat=tr.concat, act1=tr.act1,
                                                     nan_empty=False, index=tr.embed_index))
    assert bool((tr.frontier.pos == -1).all())


def test_the_constructor_refuses_a_bad_index(setup):
    s = setup
    index, rows, _ = s["indices"]["node_degree"]
    with pytest.raises(native.SageError):
        ExactBatchEmbedTrainer(s["rowptr"], s["col"], CLASSES, index, rows - 1, 8)                  # an index past the embedding's rows
    with pytest.raises(native.SageError):
        ExactBatchEmbedTrainer(s["rowptr"], s["col"], CLASSES, index[:-1].contiguous(), rows, 8)
    with pytest.raises(native.SageError, match="concat"):
        ExactBatchEmbedTrainer(s["rowptr"], s["col"], CLASSES, index, rows, 8, gcn=False, sparse_embed=True)


def test_memory_follows_the_batch_not_the_table():
    """2^18 nodes, nearly all isolated, 64 seeds, a 1hot embedding of 2^18 x 64 with sparse_embed: one step allocates less than ONE
    [embed_rows, embed_dim] float array above what was allocated before it -- a dense gradient alone would break that."""
    n, dim, live = 1 << 18, 64, 4096
    rng = np.random.default_rng(0)
    deg = np.zeros(n, dtype=np.int64)
    deg[:live] = rng.integers(1, 9, live)
    rowptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(deg, out=rowptr[1:])
    col = rng.integers(0, live, int(rowptr[-1])).astype(np.int32)
    rp, cl = CSRGraph(rowptr, col, n).to(DEV)
    index, rows = one_hot_index(n, DEV)
    tr = ExactBatchEmbedTrainer(rp, cl, CLASSES, index, rows, dim, hidden1=32, hidden2=64, sparse_embed=True)
    seeds = torch.from_numpy(np.concatenate([rng.choice(live, 60, replace=False), live + np.arange(4)]).astype(np.int32)).to(DEV)
    tgt = torch.from_numpy(rng.integers(0, CLASSES, 64)).to(DEV)
    tr.step(seeds, tgt)                                                # warm-up: the scratch buffers exist now
    old = tr.embed.clone()
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    loss = tr.step(seeds, tgt)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated()
    table = 4 * rows * dim
    print(f"allocated before the step {before} bytes, peak {peak}, above it {peak - before}; one [embed_rows, embed_dim] array {table}")
    assert bool(torch.isfinite(loss))
    assert peak - before < table, f"a step allocated {peak - before} bytes above {before}: as much as an [embed_rows, embed_dim] array ({table})"
    moved = (tr.embed != old).any(1)
    assert 0 < int(moved.sum()) <= live and not bool(moved[live:].any()), "rows of nodes outside the batch's neighbourhood were written"


def _cora():
    z = np.load(os.path.join(GOLDEN_DIR, "cora_topology.npz"))
    g = CSRGraph(z["rowptr"], z["col"], len(z["rowptr"]) - 1)
    _, labels = standin_citation(g, num_classes=7, feat_dim=64, seed=0)
    return g, labels


@pytest.mark.parametrize("initializer,sparse", [("1hot", False), ("1hot", True), ("node_degree", False)])
def test_run_exact_batch_training_trains_an_embedding_on_the_cora_standin(initializer, sparse):
    g, labels = _cora()
    torch.manual_seed(0)
    res = run_exact_batch_training(g, None, labels, 7, seed=1, epochs=5, batch_size=256, initializer=initializer, sparse_embed=sparse)
    losses, tr = res["losses"], res["trainer"]
    q = max(len(losses) // 4, 1)
    first, last = float(np.mean(losses[:q])), float(np.mean(losses[-q:]))
    print(f"{initializer} sparse={sparse} on stand-in Cora: {len(losses)} steps, mean loss {first:.4f} -> {last:.4f}, F1 micro "
          f"{res['f1_micro']:.3f} macro {res['f1_macro']:.3f}, {res['mean_step_time'] * 1e3:.3f} ms per step")
    assert isinstance(tr, ExactBatchEmbedTrainer) and tr.sparse_embed == sparse
    assert tr.act1 == (ACT_SIGMOID if initializer == "node_degree" else ACT_RELU) and tr.embed.shape[1] == 100
    assert tr.embed.shape[0] == (g.num_nodes if initializer == "1hot" else int(g.degrees().max()) + 1)
    assert set(res) == {"f1_micro", "f1_macro", "mean_step_time", "losses", "trainer"}
    assert len(losses) == 45 and np.all(np.isfinite(losses)) and last < first, (first, last)
    assert all(bool(torch.isfinite(w).all()) for w in tr.parameters())
