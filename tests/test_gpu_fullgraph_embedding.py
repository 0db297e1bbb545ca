"""Whole-graph training with a TRAINABLE embedding at layer 1 (the 1hot / node_degree initializers, aggregators.py:30-31, 68-71):
gradients of (w1, w2, w_cls, embed) against fp64 torch autograd of the dense expression, the forward bit for bit against the
whole-graph inference on embed[index], run-to-run bit identity, and that training lowers the loss."""
import numpy as np
import pytest
import torch

from sage355 import native
from sage355.datasets import standin_citation
from sage355.fullgraph import FullGraphTrainer, degree_index, one_hot_index, run_full_graph_training
from sage355.graph import rmat_graph
from sage355.inference import embed_all_nodes
from sage355.native import ACT_RELU, ACT_SIGMOID

pytestmark = pytest.mark.gpu
DEV = "cuda"
CLASSES, TRAIN = 5, 300
H1 = {64: 32, 50: 30}                                              # 50 -> 30: one float per lane in every csr kernel


@pytest.fixture(scope="module")
def setup():
    graph = rmat_graph(13, 60_000, seed=4, accel=None)
    deg = graph.degrees()
    sizes = np.bincount(deg)
    # the degree grouping holds rows of several chunks (chunk pass + chunk-order adds), of one chunk, and empty ones
    assert graph.num_nodes == 8192 and int(deg.max()) == 1433 and sorted(sizes.tolist())[-3:] == [717, 1210, 2610]
    assert int((sizes == 0).sum()) == 1287 and int(sizes.max()) > 2 * native.CSR_MEAN_CHUNK
    rs = np.random.default_rng(2)
    ids = rs.choice(graph.num_nodes, TRAIN, replace=False)            # distinct; isolated nodes among them
    assert int((deg[ids] == 0).sum()) > 0
    labels = torch.from_numpy(rs.integers(0, CLASSES, TRAIN))
    rowptr, col = graph.to(DEV)
    n = graph.num_nodes
    src = torch.from_numpy(np.repeat(np.arange(n), np.diff(graph.rowptr)))
    dst = torch.from_numpy(graph.col.astype(np.int64))
    cnt = torch.from_numpy(deg.astype(np.float64))
    inv = torch.where(cnt > 0, 1.0 / cnt.clamp_min(1.0), torch.zeros_like(cnt))
    indices = {"identity": one_hot_index(n, DEV), "degree": degree_index(rowptr), "zero": (torch.zeros(n, dtype=torch.int32, device=DEV), 1)}
    assert indices["degree"][1] == 1434 and np.array_equal(indices["degree"][0].cpu().numpy(), deg)
    return dict(graph=graph, rowptr=rowptr, col=col, ids=ids, labels=labels, src=src, dst=dst, inv=inv, indices=indices,
                dev_ids=torch.from_numpy(ids.astype(np.int32)).to(DEV), dev_labels=labels.to(DEV))


def _trainer(s, which, gcn, act1, dim, seed=3, **kw):
    index, rows = s["indices"][which]
    torch.manual_seed(seed)
    return FullGraphTrainer(s["rowptr"], s["col"], None, CLASSES, hidden1=H1[dim], hidden2=64, gcn=gcn, embed_index=index, embed_rows=rows,
                            embed_dim=dim, act1=act1, **kw)


def _autograd_reference(s, tr, index):
    """fp64 torch autograd of the dense expression: X = embed[index], mean by index_add over the edges (zeros for an empty set),
    concat, W.x, the layer's activation, classifier, cross_entropy on the training rows."""
    src, dst, inv = s["src"], s["dst"], s["inv"]

    def mean(x):
        return torch.zeros_like(x).index_add(0, src, x[dst]) * inv[:, None]

    w1, w2, wc, emb = (w.detach().cpu().double().requires_grad_(True) for w in tr.parameters())
    x = emb[index.cpu().long()]
    agg1 = mean(x)
    pre1 = (torch.cat([x, agg1], 1) if tr.concat else agg1) @ w1.t()
    h1 = torch.sigmoid(pre1) if tr.act1 == ACT_SIGMOID else torch.relu(pre1)
    agg2 = mean(h1)
    out = torch.relu((torch.cat([h1, agg2], 1) if tr.concat else agg2) @ w2.t())
    loss = torch.nn.functional.cross_entropy(out[torch.from_numpy(s["ids"])] @ wc.t(), s["labels"])
    return loss.item(), torch.autograd.grad(loss, (w1, w2, wc, emb))


@pytest.mark.parametrize("dim", [64, 50])
@pytest.mark.parametrize("act1", [ACT_RELU, ACT_SIGMOID], ids=["relu", "sigmoid"])
@pytest.mark.parametrize("gcn", [True, False])
@pytest.mark.parametrize("which", ["identity", "degree", "zero"])
def test_embedding_gradients_match_fp64_autograd(setup, which, gcn, act1, dim):
    tr = _trainer(setup, which, gcn, act1, dim)
    assert tr.identity == (which == "identity") and tr.embed.shape == (setup["indices"][which][1], dim)
    loss, grads = tr.grads(setup["dev_ids"], setup["dev_labels"])
    assert len(grads) == 4 and grads[3].shape == tr.embed.shape
    ref_loss, ref = _autograd_reference(setup, tr, setup["indices"][which][0])
    print(f"loss {loss.item():.8f} ref {ref_loss:.8f}")
    errs = {}
    for name, g, r in zip(("w1", "w2", "w_cls", "embed"), grads, ref):
        errs[name] = (g.cpu().double() - r).abs().max().item() / r.abs().max().item()
    print("max |g - ref| / max|ref|:", {k: f"{v:.2e}" for k, v in errs.items()})
    assert abs(loss.item() - ref_loss) <= 1e-5 * max(1.0, abs(ref_loss))
    for name, err in errs.items():
        assert err <= 2e-5, f"grad {name}: max |g - ref| / max|ref| = {err:.2e}"
    if which == "degree":                                           # a degree nobody has: its embedding row gets exact zeros
        empty = torch.from_numpy(np.bincount(setup["graph"].degrees(), minlength=tr.embed.shape[0]) == 0)
        assert int(empty.sum()) == 1287 and not bool(grads[3].cpu()[empty].any())


@pytest.mark.parametrize("which,gcn,act1,dim", [("degree", True, ACT_SIGMOID, 64), ("degree", False, ACT_RELU, 50),
                                                ("identity", False, ACT_SIGMOID, 64), ("zero", True, ACT_RELU, 50)])
def test_embedding_forward_is_the_inference_forward_bit_for_bit(setup, which, gcn, act1, dim):
    tr = _trainer(setup, which, gcn, act1, dim, seed=4)
    table = tr.embed[setup["indices"][which][0].long()].contiguous()
    want = embed_all_nodes(setup["rowptr"], setup["col"], table, tr.w1, tr.w2, concat=not gcn, act1=act1, nan_empty=False,
                           rows_per_call=setup["graph"].num_nodes)
    got = tr.forward()
    assert not bool(torch.isnan(got).any())
    assert torch.equal(got.view(torch.int32), want.view(torch.int32)), "forward() differs from embed_all_nodes(table=embed[index])"


@pytest.mark.parametrize("which,gcn,act1,head", [("degree", True, ACT_SIGMOID, "native"), ("identity", False, ACT_RELU, "torch"),
                                                 ("zero", False, ACT_SIGMOID, "native")])
def test_embedding_training_is_reproducible_bit_for_bit(setup, which, gcn, act1, head):
    runs = []
    for _ in range(2):
        tr = _trainer(setup, which, gcn, act1, 64, seed=9, lr=0.3, head=head)
        losses = [tr.step(setup["dev_ids"], setup["dev_labels"]).clone() for _ in range(5)]
        runs.append((torch.stack(losses), [w.clone() for w in tr.parameters()]))
    (la, wa), (lb, wb) = runs
    assert torch.equal(la.view(torch.int32), lb.view(torch.int32)), (la.tolist(), lb.tolist())
    assert len(wa) == 4
    for name, a, b in zip(("w1", "w2", "w_cls", "embed"), wa, wb):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f"{name}: two runs differ at {int((a != b).sum())} elements"
    assert bool(torch.isfinite(la).all())


@pytest.mark.parametrize("gcn", [True, False])
def test_weights_start_as_the_frozen_table_trainer_starts_them(setup, gcn):
    tr = _trainer(setup, "degree", gcn, ACT_RELU, 64, seed=11)
    torch.manual_seed(11)
    frozen = FullGraphTrainer(setup["rowptr"], setup["col"], torch.zeros(setup["graph"].num_nodes, 64, device=DEV), CLASSES, hidden1=H1[64],
                              hidden2=64, gcn=gcn)
    assert len(frozen.parameters()) == 3 and len(tr.parameters()) == 4 and tr.parameters()[3] is tr.embed
    for a, b in zip(tr.parameters(), frozen.parameters()):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    # nn.Embedding's start (aggregators.py:31): N(0, 1)
    assert abs(float(tr.embed.mean())) < 0.02 and abs(float(tr.embed.std()) - 1.0) < 0.02


def test_table_and_embedding_are_alternatives(setup):
    index, rows = setup["indices"]["degree"]
    n = setup["graph"].num_nodes
    with pytest.raises(native.SageError):
        FullGraphTrainer(setup["rowptr"], setup["col"], torch.zeros(n, 8, device=DEV), CLASSES, embed_index=index, embed_rows=rows, embed_dim=8)
    with pytest.raises(native.SageError):
        FullGraphTrainer(setup["rowptr"], setup["col"], None, CLASSES, embed_index=index, embed_rows=rows - 1, embed_dim=8)   # index out of range
    with pytest.raises(native.SageError):
        FullGraphTrainer(setup["rowptr"], setup["col"], None, CLASSES, embed_index=index[:-1].contiguous(), embed_rows=rows, embed_dim=8)
    with pytest.raises(native.SageError):
        FullGraphTrainer(setup["rowptr"], setup["col"], None, CLASSES, embed_index=index, embed_rows=rows, embed_dim=8, act1=native.ACT_NONE)
    tr = _trainer(setup, "degree", True, ACT_RELU, 50)
    with pytest.raises(native.SageError):
        tr.refresh_table()


@pytest.mark.parametrize("initializer", ["node_degree", "1hot"])
def test_training_an_embedding_lowers_the_loss_on_standin_citation(setup, initializer):
    graph = setup["graph"]
    _, labels = standin_citation(graph, num_classes=7, feat_dim=64, seed=0)
    torch.manual_seed(0)
    res = run_full_graph_training(graph, None, labels, 7, seed=1, steps=30, initializer=initializer, embed_dim=32)
    tr, losses = res["trainer"], res["losses"]
    print(initializer, "losses:", [f"{x:.4f}" for x in losses], "f1_micro", res["f1_micro"])
    assert tr.act1 == (ACT_SIGMOID if initializer == "node_degree" else ACT_RELU) and tr.identity == (initializer == "1hot")
    assert tr.embed.shape == ((graph.num_nodes if initializer == "1hot" else 1434), 32)
    assert len(losses) == 30 and all(np.isfinite(losses)) and losses[-1] < losses[0], losses
    assert all(bool(torch.isfinite(w).all()) for w in tr.parameters())
