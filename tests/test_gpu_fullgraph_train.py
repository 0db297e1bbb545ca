"""Whole-graph training (sage355.fullgraph.FullGraphTrainer): full neighbourhoods at both layers, the backward through
sage_csr_mean_backward.  Gradients against fp64 torch autograd of the dense expression, the forward bit for bit against the
whole-graph inference it serves, run-to-run bit identity, and that training lowers the loss."""
import numpy as np
import pytest
import torch

from sage355 import native
from sage355.datasets import standin_citation
from sage355.fullgraph import FullGraphTrainer
from sage355.graph import rmat_graph
from sage355.inference import embed_all_nodes

pytestmark = pytest.mark.gpu
DEV = "cuda"
CLASSES, TRAIN = 5, 300


@pytest.fixture(scope="module")
def setup():
    graph = rmat_graph(11, 30_000, seed=4, accel=None)                 # 2048 nodes, a hub of 768 entries, 333 isolated nodes
    deg = graph.degrees()
    assert graph.num_nodes == 2048 and int(deg.max()) > native.CSR_MEAN_CHUNK and int((deg == 0).sum()) > 0
    rs = np.random.default_rng(2)
    ids = rs.choice(graph.num_nodes, TRAIN, replace=False)            # distinct; isolated nodes and the hub's neighbours among them
    labels = torch.from_numpy(rs.integers(0, CLASSES, TRAIN))
    rowptr, col = graph.to(DEV)
    tables = {d0: torch.randn(graph.num_nodes, d0, generator=torch.Generator().manual_seed(d0)) for d0 in (64, 50, 256)}
    return graph, rowptr, col, ids, labels, tables


def _autograd_reference(graph, table, tr, ids, labels):
    """fp64 torch autograd of the dense expression: mean by index_add_ over the edges (zeros for an empty set), concat, W.x, relu,
    classifier, cross_entropy on the training rows."""
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
@pytest.mark.parametrize("d0,h1", [(64, 32), (50, 30), (256, 128)])     # (50, 30): one float per lane in both csr_mean kernels
@pytest.mark.parametrize("gcn", [True, False])
def test_fullgraph_gradients_match_fp64_autograd(setup, gcn, d0, h1, self_loop, head):
    graph, rowptr, col, ids, labels, tables = setup
    torch.manual_seed(3)
    tr = FullGraphTrainer(rowptr, col, tables[d0].to(DEV), CLASSES, hidden1=h1, hidden2=64, gcn=gcn, agg_self_loop=self_loop, head=head)
    loss, grads = tr.grads(torch.from_numpy(ids.astype(np.int32)).to(DEV), labels.to(DEV))
    ref_loss, ref = _autograd_reference(graph, tables[d0], tr, ids, labels)
    print(f"loss {loss.item():.8f} ref {ref_loss:.8f}")
    errs = {}
    for name, g, r in zip(("w1", "w2", "w_cls"), grads, ref):
        errs[name] = (g.cpu().double() - r).abs().max().item() / r.abs().max().item()
    print("max |g - ref| / max|ref|:", {k: f"{v:.2e}" for k, v in errs.items()})
    assert abs(loss.item() - ref_loss) <= 1e-5 * max(1.0, abs(ref_loss))
    for name, err in errs.items():
        assert err <= 2e-5, f"grad {name}: max |g - ref| / max|ref| = {err:.2e}"


@pytest.mark.parametrize("gcn,d0,h1,self_loop", [(True, 64, 32, False), (False, 50, 30, True), (False, 256, 128, False)])
def test_fullgraph_forward_is_the_inference_forward_bit_for_bit(setup, gcn, d0, h1, self_loop):
    graph, rowptr, col, ids, labels, tables = setup
    torch.manual_seed(4)
    table = tables[d0].to(DEV)
    tr = FullGraphTrainer(rowptr, col, table, CLASSES, hidden1=h1, hidden2=64, gcn=gcn, agg_self_loop=self_loop)
    want = embed_all_nodes(rowptr, col, table, tr.w1, tr.w2, concat=not gcn, agg_self_loop=self_loop, nan_empty=False,
                           rows_per_call=graph.num_nodes)
    got = tr.forward()
    assert not bool(torch.isnan(got).any())
    assert torch.equal(got.view(torch.int32), want.view(torch.int32)), "forward() differs from embed_all_nodes(nan_empty=False)"


@pytest.mark.parametrize("gcn,head", [(True, "native"), (False, "torch")])
def test_fullgraph_training_is_reproducible_bit_for_bit(setup, gcn, head):
    graph, rowptr, col, ids, labels, tables = setup
    table = tables[64].to(DEV)
    dev_ids, dev_labels = torch.from_numpy(ids.astype(np.int32)).to(DEV), labels.to(DEV)
    runs = []
    for _ in range(2):
        torch.manual_seed(9)
        tr = FullGraphTrainer(rowptr, col, table, CLASSES, hidden1=32, hidden2=64, gcn=gcn, lr=0.3, agg_self_loop=True, head=head)
        losses = [tr.step(dev_ids, dev_labels).clone() for _ in range(5)]
        runs.append((torch.stack(losses), [w.clone() for w in tr.parameters()]))
    (la, wa), (lb, wb) = runs
    assert torch.equal(la.view(torch.int32), lb.view(torch.int32)), (la.tolist(), lb.tolist())
    for name, a, b in zip(("w1", "w2", "w_cls"), wa, wb):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f"{name}: two runs differ at {int((a != b).sum())} elements"
    assert bool(torch.isfinite(la).all())


def test_fullgraph_training_lowers_the_loss_on_standin_citation(setup):
    graph = setup[0]
    feats, labels = standin_citation(graph, num_classes=7, feat_dim=1433, seed=0)
    rowptr, col = setup[1], setup[2]
    n = graph.num_nodes
    train = np.random.default_rng(1).permutation(n)[int(0.2 * n):]
    ids = torch.from_numpy(train.astype(np.int32)).to(DEV)
    tgt = torch.from_numpy(np.asarray(labels).reshape(-1))[torch.from_numpy(train)].to(DEV)
    torch.manual_seed(0)
    tr = FullGraphTrainer(rowptr, col, torch.from_numpy(feats).to(DEV), 7)
    losses = [float(tr.step(ids, tgt)) for _ in range(30)]
    print("losses:", [f"{x:.4f}" for x in losses])
    assert losses[-1] < losses[0], losses
    assert all(bool(torch.isfinite(w).all()) for w in tr.parameters())
    pred = tr.predict(ids)
    assert pred.dtype == torch.int32 and pred.shape == ids.shape and int(pred.min()) >= 0 and int(pred.max()) < 7
