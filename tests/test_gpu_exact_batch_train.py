"""Exact mini-batch training (sage355.exactbatch.ExactBatchTrainer): full neighbourhoods at both layers for a seed batch, the
backward through sage_csr_mean_backward_rows.  The setup is tests/test_gpu_fullgraph_train.py's: the forward bit for bit against
embed_nodes and the whole-graph trainer, the loss and the classifier's gradient bit for bit against the whole-graph trainer, the
gradients of w1 and w2 against fp64 torch autograd of the dense expression at that file's bars (max |g - ref| / max|ref| <= 2e-5,
loss 1e-5: the same expression summed over fewer rows), run-to-run bit identity, the state of the id -> row map after a step,
memory that follows the batch and not the graph, and that training lowers the loss."""
import numpy as np
import pytest
import torch

from sage355 import native
from sage355.datasets import standin_citation
from sage355.exactbatch import ExactBatchTrainer, run_exact_batch_training
from sage355.fullgraph import FullGraphTrainer
from sage355.graph import CSRGraph, rmat_graph
from sage355.inference import embed_nodes

pytestmark = pytest.mark.gpu
DEV = "cuda"
CLASSES, TRAIN = 5, 300


def bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.fixture(scope="module")
def setup():
    graph = rmat_graph(11, 30_000, seed=4, accel=None)                 # 2048 nodes, a hub of 768 entries, 333 isolated nodes
    deg = graph.degrees()
    assert graph.num_nodes == 2048 and int(deg.max()) > native.CSR_MEAN_CHUNK and int((deg == 0).sum()) > 0
    rs = np.random.default_rng(2)
    ids = rs.choice(graph.num_nodes, TRAIN, replace=False)            # distinct; isolated nodes and the hub's neighbours among them
    assert (deg[ids] == 0).any()
    labels = torch.from_numpy(rs.integers(0, CLASSES, TRAIN))
    rowptr, col = graph.to(DEV)
    tables = {d0: torch.randn(graph.num_nodes, d0, generator=torch.Generator().manual_seed(d0)) for d0 in (64, 50, 256)}
    return graph, rowptr, col, ids, labels, tables


def _autograd_reference(graph, table, tr, ids, labels):
    """fp64 torch autograd of the dense expression (tests/test_gpu_fullgraph_train.py): mean by index_add_ over the edges (zeros for
    an empty set), concat, W.x, relu, classifier, cross_entropy on the training rows."""
    n = graph.num_nodes
    deg = np.diff(graph.rowptr)
    src = torch.from_numpy(np.repeat(np.arange(n), deg))
    dst = torch.from_numpy(graph.col.astype(np.int64))
    own = np.zeros(n, dtype=bool)
    own[src[dst == src].numpy()] = True
    extra = torch.from_numpy((~own) if tr.self_loop else np.zeros(n, dtype=bool))
    cnt = torch.from_numpy(deg.astype(np.float64)) + extra.double()
    inv = torch.where(cnt > 0, 1.0 / cnt.clamp_min(1.0), torch.zeros_like(cnt))

    def mean(x):
        s = torch.zeros_like(x).index_add(0, src, x[dst])
        return (s + x * extra.double()[:, None]) * inv[:, None]

    t64 = table.double()
    w1, w2, wc = (w.detach().cpu().double().requires_grad_(True) for w in tr.parameters())
    agg1 = mean(t64)
    h1 = torch.relu((torch.cat([t64, agg1], 1) if tr.concat else agg1) @ w1.t())
    agg2 = mean(h1)
    out = torch.relu((torch.cat([h1, agg2], 1) if tr.concat else agg2) @ w2.t())
    loss = torch.nn.functional.cross_entropy(out[torch.from_numpy(ids)] @ wc.t(), labels)
    return loss.item(), torch.autograd.grad(loss, (w1, w2, wc))


@pytest.mark.parametrize("head", ["native", "torch"])
@pytest.mark.parametrize("self_loop", [False, True])
@pytest.mark.parametrize("d0,h1", [(64, 32), (50, 30), (256, 128)])
@pytest.mark.parametrize("gcn", [True, False])
def test_exact_batch_forward_loss_and_gradients(setup, gcn, d0, h1, self_loop, head):
    graph, rowptr, col, ids, labels, tables = setup
    table = tables[d0].to(DEV)
    seeds, tgt = torch.from_numpy(ids.astype(np.int32)).to(DEV), labels.to(DEV)
    kw = dict(hidden1=h1, hidden2=64, gcn=gcn, agg_self_loop=self_loop, head=head)
    torch.manual_seed(3)
    tr = ExactBatchTrainer(rowptr, col, table, CLASSES, **kw)
    torch.manual_seed(3)
    full = FullGraphTrainer(rowptr, col, table, CLASSES, **kw)
    for a, b in zip(tr.parameters(), full.parameters()):
        assert bits_equal(a, b), "one torch seed must give both trainers the same start"
    # the forward: embed_nodes' bits and the whole-graph trainer's
    got = tr.forward(seeds)
    assert not bool(torch.isnan(got).any())
    assert bits_equal(got, embed_nodes(rowptr, col, table, tr.w1, tr.w2, seeds, concat=not gcn, agg_self_loop=self_loop, nan_empty=False))
    assert bits_equal(got, full.forward()[seeds.long()]), "forward(seeds) differs from FullGraphTrainer.forward()[seeds]"
    # the head sees the same rows in the same order: loss and dW_cls bit for bit
    loss, grads = tr.grads(seeds, tgt)
    full_loss, full_grads = full.grads(seeds, tgt)
    assert bits_equal(loss.reshape(1), full_loss.reshape(1)), (loss.item(), full_loss.item())
    assert bits_equal(grads[2], full_grads[2]), "the gradient of w_cls differs from the whole-graph trainer's"
    assert bool((tr.frontier.pos == -1).all()), "the map is not clear after grads()"
    # w1, w2 (and w_cls again) against fp64
    ref_loss, ref = _autograd_reference(graph, tables[d0], tr, ids, labels)
    print(f"loss {loss.item():.8f} ref {ref_loss:.8f}")
    errs = {}
    for name, g, r in zip(("w1", "w2", "w_cls"), grads, ref):
        errs[name] = (g.cpu().double() - r).abs().max().item() / r.abs().max().item()
    print("max |g - ref| / max|ref|:", {k: f"{v:.2e}" for k, v in errs.items()})
    assert abs(loss.item() - ref_loss) <= 1e-5 * max(1.0, abs(ref_loss))
    for name, err in errs.items():
        assert err <= 2e-5, f"grad {name}: max |g - ref| / max|ref| = {err:.2e}"


@pytest.mark.parametrize("gcn,head", [(True, "native"), (False, "torch")])
def test_exact_batch_training_is_reproducible_bit_for_bit(setup, gcn, head):
    graph, rowptr, col, ids, labels, tables = setup
    table = tables[64].to(DEV)
    dev_ids, dev_labels = torch.from_numpy(ids.astype(np.int32)).to(DEV), labels.to(DEV)
    runs = []
    for _ in range(2):
        torch.manual_seed(9)
        tr = ExactBatchTrainer(rowptr, col, table, CLASSES, hidden1=32, hidden2=64, gcn=gcn, lr=0.3, agg_self_loop=True, head=head)
        losses = [tr.step(dev_ids, dev_labels).clone() for _ in range(5)]
        runs.append((torch.stack(losses), [w.clone() for w in tr.parameters()]))
    (la, wa), (lb, wb) = runs
    assert bits_equal(la, lb), (la.tolist(), lb.tolist())
    for name, a, b in zip(("w1", "w2", "w_cls"), wa, wb):
        assert bits_equal(a, b), f"{name}: two runs differ at {int((a != b).sum())} elements"
    assert bool(torch.isfinite(la).all())


def test_the_map_is_clear_after_a_step_and_after_a_step_that_raised(setup):
    graph, rowptr, col, ids, labels, tables = setup
    tr = ExactBatchTrainer(rowptr, col, tables[64].to(DEV), CLASSES, hidden1=32, hidden2=64, gcn=False)
    seeds, tgt = torch.from_numpy(ids.astype(np.int32)).to(DEV), labels.to(DEV)
    tr.step(seeds, tgt)
    assert bool((tr.frontier.pos == -1).all()) and int(tr.frontier.count) == 0
    bad = seeds.clone()
    bad[17] = graph.num_nodes + 4
    with pytest.raises(native.SageError):
        tr.step(bad, tgt)
    assert bool((tr.frontier.pos == -1).all()) and int(tr.frontier.count) == 0
    with pytest.raises(native.SageError):                              # labels of another length
        tr.grads(seeds, tgt[:-1])
    assert bool((tr.frontier.pos == -1).all())
    loss = tr.step(seeds, tgt)                                         # and the trainer still works
    assert bool(torch.isfinite(loss))
    pred = tr.predict(seeds)
    assert pred.dtype == torch.int32 and pred.shape == seeds.shape and int(pred.min()) >= 0 and int(pred.max()) < CLASSES
    assert bool((tr.frontier.pos == -1).all())


def test_memory_follows_the_batch_not_the_graph():
    """2^18 nodes, nearly all isolated, 64 seeds, h1 = 128: one step allocates less than ONE [N, h1] float array (4 N h1 bytes)
    above what was allocated before it -- a whole-graph hidden array alone would break that."""
    n, h1, live = 1 << 18, 128, 4096
    rng = np.random.default_rng(0)
    deg = np.zeros(n, dtype=np.int64)
    deg[:live] = rng.integers(1, 9, live)
    rowptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(deg, out=rowptr[1:])
    col = rng.integers(0, live, int(rowptr[-1])).astype(np.int32)
    rp, cl = CSRGraph(rowptr, col, n).to(DEV)
    table = torch.randn(n, 16, device=DEV)
    tr = ExactBatchTrainer(rp, cl, table, CLASSES, hidden1=h1, hidden2=64)
    seeds = torch.from_numpy(np.concatenate([rng.choice(live, 60, replace=False), live + np.arange(4)]).astype(np.int32)).to(DEV)
    tgt = torch.from_numpy(rng.integers(0, CLASSES, 64)).to(DEV)
    tr.step(seeds, tgt)                                                # warm-up: the scratch buffers exist now
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    loss = tr.step(seeds, tgt)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated()
    print(f"allocated before the step {before} bytes, peak {peak}, above it {peak - before}; one [N, h1] array {4 * n * h1}")
    assert bool(torch.isfinite(loss))
    assert peak - before < 4 * n * h1, f"a step allocated {peak - before} bytes above {before}: as much as an [N, h1] array ({4 * n * h1})"


def test_run_exact_batch_training_lowers_the_loss_on_standin_citation(setup):
    graph = setup[0]
    feats, labels = standin_citation(graph, num_classes=7, feat_dim=1433, seed=0)
    torch.manual_seed(0)
    res = run_exact_batch_training(graph, feats, labels, 7, seed=1, epochs=3, batch_size=128)
    losses = res["losses"]
    print("losses:", [f"{x:.4f}" for x in losses[:30]])
    assert len(losses) >= 30 and set(res) == {"f1_micro", "f1_macro", "mean_step_time", "losses", "trainer"}
    # mini-batch losses scatter: the mean of the last five of the first 30 steps against the mean of the first five
    assert np.mean(losses[25:30]) < np.mean(losses[:5]), losses[:30]
    assert all(bool(torch.isfinite(w).all()) for w in res["trainer"].parameters())
    assert 0.0 <= res["f1_micro"] <= 1.0
