"""FullGraphTrainer(fused_embed=True): layer 1 reads the trainable embedding through the index in both directions (the indexed
mean, self_index, the grouped backward) and X = embed[index] is never built.  Against fused_embed=False from one seed: forward(),
the loss and the gradients of w2 and w_cls bit for bit; the gradients of w1 and embed against fp64 torch autograd of the dense
expression at the bars of tests/test_gpu_fullgraph_embedding.py (2e-5 of the reference's maximum; loss 1e-5); whether w1 also
comes out bit-equal is printed.  The R-MAT graph is that file's (8,192 nodes; fixture copied)."""
import numpy as np
import pytest
import torch

from sage355 import native
from sage355.datasets import standin_citation
from sage355.fullgraph import FullGraphTrainer, degree_index, one_hot_index, run_full_graph_training
from sage355.graph import rmat_graph
from sage355.native import ACT_RELU, ACT_SIGMOID

pytestmark = pytest.mark.gpu
DEV = "cuda"
CLASSES, TRAIN = 5, 300
H1 = {64: 32, 50: 30}
NAMES = ("w1", "w2", "w_cls", "embed")


def bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.fixture(scope="module")
def setup():
    graph = rmat_graph(13, 60_000, seed=4, accel=None)
    deg = graph.degrees()
    sizes = np.bincount(deg)
    assert graph.num_nodes == 8192 and int(deg.max()) == 1433 and int((sizes == 0).sum()) == 1287 and int(sizes.max()) > 2 * native.CSR_MEAN_CHUNK
    rs = np.random.default_rng(2)
    ids = rs.choice(graph.num_nodes, TRAIN, replace=False)            # distinct; isolated nodes among them
    assert int((deg[ids] == 0).sum()) > 0
    labels = torch.from_numpy(rs.integers(0, CLASSES, TRAIN))
    rowptr, col = graph.to(DEV)
    n = graph.num_nodes
    src = torch.from_numpy(np.repeat(np.arange(n), np.diff(graph.rowptr)))
    dst = torch.from_numpy(graph.col.astype(np.int64))
    own = np.zeros(n, dtype=bool)
    own[src[dst == src].numpy()] = True
    indices = {"identity": one_hot_index(n, DEV), "degree": degree_index(rowptr), "zero": (torch.zeros(n, dtype=torch.int32, device=DEV), 1)}
    return dict(graph=graph, rowptr=rowptr, col=col, ids=ids, labels=labels, src=src, dst=dst, deg=deg, own=own, indices=indices,
                dev_ids=torch.from_numpy(ids.astype(np.int32)).to(DEV), dev_labels=labels.to(DEV))


def _trainer(s, which, gcn, act1, dim, fused, seed=3, **kw):
    index, rows = s["indices"][which]
    torch.manual_seed(seed)
    return FullGraphTrainer(s["rowptr"], s["col"], None, CLASSES, hidden1=H1[dim], hidden2=64, gcn=gcn, embed_index=index, embed_rows=rows,
                            embed_dim=dim, act1=act1, fused_embed=fused, **kw)


def _autograd_reference(s, tr, index):
    """fp64 torch autograd of the dense expression (tests/test_gpu_fullgraph_embedding.py), with the set-union self term when the
    trainer's aggregator adds it."""
    src, dst = s["src"], s["dst"]
    extra = torch.from_numpy(~s["own"] if tr.self_loop else np.zeros_like(s["own"])).double()
    cnt = torch.from_numpy(s["deg"].astype(np.float64)) + extra
    inv = torch.where(cnt > 0, 1.0 / cnt.clamp_min(1.0), torch.zeros_like(cnt))

    def mean(x):
        return (torch.zeros_like(x).index_add(0, src, x[dst]) + x * extra[:, None]) * inv[:, None]

    w1, w2, wc, emb = (w.detach().cpu().double().requires_grad_(True) for w in tr.parameters())
    x = emb[index.cpu().long()]
    agg1 = mean(x)
    pre1 = (torch.cat([x, agg1], 1) if tr.concat else agg1) @ w1.t()
    h1 = torch.sigmoid(pre1) if tr.act1 == ACT_SIGMOID else torch.relu(pre1)
    agg2 = mean(h1)
    out = torch.relu((torch.cat([h1, agg2], 1) if tr.concat else agg2) @ w2.t())
    loss = torch.nn.functional.cross_entropy(out[torch.from_numpy(s["ids"])] @ wc.t(), s["labels"])
    return loss.item(), torch.autograd.grad(loss, (w1, w2, wc, emb))


@pytest.mark.parametrize("self_loop", [False, True], ids=["", "selfloop"])
@pytest.mark.parametrize("dim", [64, 50])
@pytest.mark.parametrize("act1", [ACT_RELU, ACT_SIGMOID], ids=["relu", "sigmoid"])
@pytest.mark.parametrize("gcn", [True, False], ids=["gcn", "concat"])
@pytest.mark.parametrize("which", ["identity", "degree", "zero"])
def test_fused_step_against_the_unfused_one_and_fp64_autograd(setup, which, gcn, act1, dim, self_loop):
    plain = _trainer(setup, which, gcn, act1, dim, False, agg_self_loop=self_loop)
    fused = _trainer(setup, which, gcn, act1, dim, True, agg_self_loop=self_loop)
    assert fused.fused == (which != "identity") and not plain.fused
    for a, b in zip(plain.parameters(), fused.parameters()):
        assert bits_equal(a, b)
    assert bits_equal(fused.forward(), plain.forward()), "forward() differs"
    loss_p, g_p = plain.grads(setup["dev_ids"], setup["dev_labels"])
    loss_f, g_f = fused.grads(setup["dev_ids"], setup["dev_labels"])
    assert len(g_f) == 4 and g_f[3].shape == fused.embed.shape
    assert bits_equal(loss_f.reshape(1), loss_p.reshape(1)), (loss_f.item(), loss_p.item())
    assert bits_equal(g_f[1], g_p[1]) and bits_equal(g_f[2], g_p[2]), "the gradients of w2 / w_cls differ"
    print(f"{which}: grad w1 bit-equal to the unfused one: {bits_equal(g_f[0], g_p[0])}; grad embed bit-equal: {bits_equal(g_f[3], g_p[3])}")
    if which == "identity":                                          # the embedding is the table already: the flag changes nothing
        assert all(bits_equal(a, b) for a, b in zip(g_f, g_p))
        assert fused.x is fused.embed
    else:
        assert fused.x is None and plain.x is not None, "a fused step must not build X"
    ref_loss, ref = _autograd_reference(setup, fused, setup["indices"][which][0])
    assert abs(loss_f.item() - ref_loss) <= 1e-5 * max(1.0, abs(ref_loss))
    errs = {name: (g.cpu().double() - r).abs().max().item() / r.abs().max().item() for name, g, r in zip(NAMES, g_f, ref)}
    print("max |g - ref| / max|ref|:", {k: f"{v:.2e}" for k, v in errs.items()})
    for name, err in errs.items():
        assert err <= 2e-5, f"grad {name}: max |g - ref| / max|ref| = {err:.2e}"
    if which == "degree":                                            # a degree nobody has: its embedding row gets exact zeros
        empty = torch.from_numpy(np.bincount(setup["deg"], minlength=fused.embed.shape[0]) == 0)
        assert int(empty.sum()) == 1287 and not bool(g_f[3].cpu()[empty].any())


def test_the_default_is_unfused_and_allocates_what_it_did(setup):
    tr = _trainer(setup, "degree", False, ACT_SIGMOID, 64, False)
    default = FullGraphTrainer(setup["rowptr"], setup["col"], None, CLASSES, embed_index=setup["indices"]["degree"][0], embed_rows=1434, embed_dim=64)
    assert not tr.fused and not default.fused and default.grouped_t is None and tr.grouped_t is None
    tr.step(setup["dev_ids"], setup["dev_labels"])
    assert tr.x is not None and tuple(tr.x.shape) == (8192, 64)


@pytest.mark.parametrize("which,gcn,act1,head", [("degree", True, ACT_SIGMOID, "native"), ("degree", False, ACT_RELU, "torch"),
                                                 ("zero", False, ACT_SIGMOID, "native")])
def test_fused_training_is_reproducible_bit_for_bit(setup, which, gcn, act1, head):
    runs = []
    for _ in range(2):
        tr = _trainer(setup, which, gcn, act1, 64, True, seed=9, lr=0.3, head=head)
        losses = [tr.step(setup["dev_ids"], setup["dev_labels"]).clone() for _ in range(5)]
        assert tr.x is None
        runs.append((torch.stack(losses), [w.clone() for w in tr.parameters()]))
    (la, wa), (lb, wb) = runs
    assert bits_equal(la, lb), (la.tolist(), lb.tolist())
    for name, a, b in zip(NAMES, wa, wb):
        assert bits_equal(a, b), f"{name}: two runs differ at {int((a != b).sum())} elements"
    assert bool(torch.isfinite(la).all())


def test_fused_training_lowers_the_loss_on_standin_citation(setup):
    graph = setup["graph"]
    _, labels = standin_citation(graph, num_classes=7, feat_dim=64, seed=0)
    torch.manual_seed(0)
    res = run_full_graph_training(graph, None, labels, 7, seed=1, steps=30, initializer="node_degree", embed_dim=32, fused_embed=True)
    tr, losses = res["trainer"], res["losses"]
    print("losses:", [f"{x:.4f}" for x in losses], "f1_micro", res["f1_micro"])
    assert tr.fused and tr.x is None and tr.act1 == ACT_SIGMOID and tr.embed.shape == (1434, 32)
    assert len(losses) == 30 and all(np.isfinite(losses)) and losses[-1] < losses[0], losses
    assert all(bool(torch.isfinite(w).all()) for w in tr.parameters())
