"""EngineTrainer(sparse_embed=True): the embedding's update applied to the rows a batch touched and to nothing else.  Against the
dense trainer from the same state -- gradients, losses and weights bit for bit, the touched embedding rows to one rounding -- its
reproducibility, the forward after a sparse step (engine and a live RolePipeline), the memory a step allocates, and training."""
import os

import numpy as np
import pytest
import torch

from sage355 import native, ops
from sage355.datasets import standin_citation
from sage355.engine import RolePipeline, TwoHopEngine
from sage355.fullgraph import degree_index, one_hot_index
from sage355.graph import CSRGraph, rmat_graph
from sage355.train import EngineTrainer, run_engine_training
from util import GOLDEN_DIR

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24
KINDS = {"identity": ops.ACT_RELU, "degree": ops.ACT_SIGMOID}          # the index and the layer-1 activation it is trained with
EMBED_DIM, BATCH = 64, 256

_state = {}


def small_graph():
    """tests/test_gpu_engine_embedding.py's graph, its two indices and 1100 candidate seeds of non-zero degree, built once."""
    if not _state:
        graph = rmat_graph(13, 150_000, seed=4, accel=None)
        rowptr, col = graph.to(DEV)
        n = graph.num_nodes
        _state.update(graph=graph, rowptr=rowptr, col=col, n=n, index={"degree": degree_index(rowptr), "identity": one_hot_index(n, DEV)},
                      cand=np.random.default_rng(2).choice(np.nonzero(graph.degrees() > 0)[0], 1100, replace=False),
                      labels=torch.from_numpy(np.random.default_rng(3).integers(0, 5, n)).to(DEV))
    return _state


def batch(i):
    s = small_graph()
    ids = torch.from_numpy(s["cand"][i * BATCH:(i + 1) * BATCH].astype(np.int32)).to(DEV)
    return ids, s["labels"][ids.long()]


def trainer(kind, sparse, seed=5, lr=0.3, **kw):
    s = small_graph()
    index, rows = s["index"][kind]
    torch.manual_seed(seed)
    return EngineTrainer(s["rowptr"], s["col"], None, 5, hidden1=32, hidden2=32, num_sample1=7, num_sample2=9, lr=lr, max_batch=BATCH,
                         embed_index=index, embed_rows=rows, embed_dim=EMBED_DIM, act1=KINDS[kind], sparse_embed=sparse, **kw)


def bits(t):
    return t.contiguous().view(torch.int32)


def sampled_rows(tr):
    """bool [R]: the embedding rows in the layer-1 sets of the trainer's LAST forward."""
    it = tr.engine.intermediates()
    mask = torch.arange(it["nbr1"].shape[1], device=DEV)[None, :] < it["cnt1"][:, None]
    used = torch.zeros(tr.embed_weight.shape[0], dtype=torch.bool, device=DEV)
    used[it["nbr1"][mask].long()] = True
    return used


def one_rounding(new, old, g, lr, what):
    """|new - (old - lr g)| <= 2^-24 |old - lr g| (1 + 2^-20), the right-hand side in fp64 with lr the float32 the kernel is handed:
    one fp32 rounding of the exact value; the last factor covers the fp64 reference's own rounding."""
    ref = old.double() - float(np.float32(lr)) * g.double()
    err = (new.double() - ref).abs()
    bound = U * ref.abs() * (1 + 2.0 ** -20)
    worst = float((err / bound.clamp_min(1e-300)).max())
    print(f"{what}: max |new - ref| = {float(err.max()):.3e}, max err / bound = {worst:.3f}")
    assert bool((err <= bound).all()), f"{what}: more than one rounding away from old - lr * g (ratio {worst:.3f})"


@pytest.mark.parametrize("head", ["torch", "native"])
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_a_sparse_trainers_gradients_are_the_dense_ones(kind, head):
    dense, sparse = trainer(kind, False, head=head), trainer(kind, True, head=head)
    for x, y in zip(dense.parameters(), sparse.parameters()):
        assert torch.equal(x, y)
    ids, labels = batch(0)
    loss_d, gd = dense.grads(ids, labels, key=11)
    loss_s, gs = sparse.grads(ids, labels, key=11)
    assert torch.equal(bits(loss_d.reshape(1)), bits(loss_s.reshape(1))) and len(gd) == len(gs) == 4
    for name, x, y in zip(("w1", "w2", "w_cls"), gd, gs):
        assert torch.equal(bits(x), bits(y)), f"grad {name} differs between the dense and the sparse trainer"
    rows, num, grad_rows = gs[3]
    rows_n = dense.embed_weight.shape[0]
    u = int(num)
    cap = min(sparse.engine.layout.max_s1 * 7, rows_n)
    assert rows.shape == (cap,) and grad_rows.shape == (cap, EMBED_DIM) and 0 < u <= cap
    used = sampled_rows(sparse)
    assert torch.equal(rows[:u].long(), torch.nonzero(used)[:, 0]), "rows are not the sampled embedding rows, ascending"
    scattered = torch.zeros(rows_n, EMBED_DIM, device=DEV)
    scattered[rows[:u].long()] = grad_rows[:u]
    assert torch.equal(bits(scattered), bits(gd[3])), "the compact gradient scattered into zeros is not the dense gradient"
    for p, q in zip(dense.parameters(), sparse.parameters()):
        assert torch.equal(p, q), "grads() must update nothing"
    # the engine's forms beside each other: the weight gradients do not depend on the form, the buffers are the engine's own
    e = sparse.engine
    out = e.forward(ids, seed=11)
    cot = torch.randn(out.shape, generator=torch.Generator().manual_seed(1)).to(DEV)
    a1, a2, a3 = e.backward_weights(out, cot, need_embed=True)
    b1, b2, (r, n, g) = e.backward_weights(out, cot, need_embed="rows")
    assert torch.equal(a1, b1) and torch.equal(a2, b2) and r.data_ptr() == rows.data_ptr() and g.data_ptr() == grad_rows.data_ptr()
    assert torch.equal(bits(a3[r[:int(n)].long()]), bits(g[:int(n)])) and int(n) == int((a3 != 0).any(1).sum())


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_a_sparse_step_is_the_dense_step_at_five_successive_states(kind):
    dense, sparse = trainer(kind, False), trainer(kind, True)
    lr = sparse.lr
    for i in range(5):
        ids, labels = batch(i % 4)
        key = 100 + i
        with torch.no_grad():
            for p, q in zip(dense.parameters(), sparse.parameters()):
                p.copy_(q)
        old = sparse.embed_weight.clone()
        g = dense.grads(ids, labels, key)[1][3].clone()                       # the dense gradient at this state
        loss_d = dense.step(ids, labels, key).clone()
        loss_s = sparse.step(ids, labels, key).clone()
        assert torch.equal(bits(loss_d.reshape(1)), bits(loss_s.reshape(1))), f"state {i}: the losses differ"
        for name, x, y in zip(("w1", "w2", "w_cls"), dense.parameters(), sparse.parameters()):
            assert torch.equal(bits(x), bits(y)), f"state {i}: {name} differs after the step"
        used = sampled_rows(sparse)
        assert torch.equal(used, sampled_rows(dense)) and bool(used.any())
        assert bool((~used).any()) or kind == "degree"
        assert torch.equal(bits(sparse.embed_weight[~used]), bits(old[~used])), f"state {i}: the sparse step wrote a row nobody sampled"
        assert torch.equal(bits(dense.embed_weight[~used]), bits(old[~used])), f"state {i}: the dense step moved a row nobody sampled"
        assert not g[~used].any()
        one_rounding(sparse.embed_weight[used], old[used], g[used], lr, f"{kind} state {i}")
        assert not torch.equal(sparse.embed_weight[used], old[used])


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_a_sparse_step_is_the_dense_step_under_the_native_head(kind):
    """The same comparison from a state four sparse steps in, with the native classifier head on both sides."""
    dense, sparse = trainer(kind, False, head="native"), trainer(kind, True, head="native")
    for i in range(4):
        ids, labels = batch(i)
        sparse.step(ids, labels, 200 + i)
    with torch.no_grad():
        for p, q in zip(dense.parameters(), sparse.parameters()):
            p.copy_(q)
    ids, labels = batch(1)
    old = sparse.embed_weight.clone()
    g = dense.grads(ids, labels, 300)[1][3].clone()
    loss_d, loss_s = dense.step(ids, labels, 300).clone(), sparse.step(ids, labels, 300).clone()
    assert torch.equal(bits(loss_d.reshape(1)), bits(loss_s.reshape(1)))
    for name, x, y in zip(("w1", "w2", "w_cls"), dense.parameters(), sparse.parameters()):
        assert torch.equal(bits(x), bits(y)), f"{name} differs after the step"
    used = sampled_rows(sparse)
    assert torch.equal(bits(sparse.embed_weight[~used]), bits(old[~used])) and torch.equal(bits(dense.embed_weight[~used]), bits(old[~used]))
    one_rounding(sparse.embed_weight[used], old[used], g[used], sparse.lr, f"{kind} fifth state")


def test_two_sparse_trainers_from_one_seed_stay_bit_identical():
    def run():
        tr = trainer("identity", True)
        first = tr.embed_weight.clone()
        losses = [tr.step(*batch(i), 100 + i).clone() for i in range(3)]
        return tr, first, losses

    a, first_a, la = run()
    b, first_b, lb = run()
    assert torch.equal(first_a, first_b) and not torch.equal(first_a, a.embed_weight)
    for x, y in zip(la, lb):
        assert torch.equal(bits(x.reshape(1)), bits(y.reshape(1))) and bool(torch.isfinite(x))
    for name, x, y in zip(("w1", "w2", "w_cls", "embed_weight"), a.parameters(), b.parameters()):
        assert torch.equal(bits(x), bits(y)), f"{name}: two runs differ at {int((x != y).sum())} elements"


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_the_next_forward_sees_a_sparse_update(kind):
    """The native update does not pass through torch: the trainer's own engine and a RolePipeline that was live across the step must
    still read the new rows (and, for the pipe, wait for them)."""
    s = small_graph()
    index, _ = s["index"][kind]
    tr = trainer(kind, True)
    kw = dict(act1=KINDS[kind], embed_index=index)
    pipe = RolePipeline(s["rowptr"], s["col"], tr.embed_weight, tr.w1, tr.w2, 7, 9, batch=BATCH, depth=2, **kw)
    ids, labels = batch(0)
    probe, _ = batch(1)

    def fresh():
        w = [p.clone() for p in tr.parameters()]
        return TwoHopEngine(s["rowptr"], s["col"], w[3], w[0], w[1], 7, 9, max_batch=BATCH, **kw).forward(probe, seed=77)

    def served():
        out = torch.zeros(BATCH, 32, device=DEV)
        pipe.submit(probe, 77, out)
        pipe.synchronize()
        return out

    before = served()
    assert torch.equal(before, fresh()) and torch.equal(before, tr.embed(probe, 77))
    version = tr.embed_weight._version
    tr.step(ids, labels, 5)
    assert tr.embed_weight._version > version, "the native update must move the embedding's version counter"
    after = fresh()
    assert not torch.equal(before, after)
    assert torch.equal(tr.embed(probe, 77), after), "the trainer's forward after a sparse step does not see the new rows"
    assert torch.equal(served(), after), "a role pipeline that was live across a sparse step does not see the new rows"
    # the embedding alone moves (the weights keep their version counters): the engine's update form, straight
    e = tr.engine
    out = e.forward(ids, seed=6)
    cot = torch.randn(out.shape, generator=torch.Generator().manual_seed(2)).to(DEV)
    versions = (tr.w1._version, tr.w2._version)
    old = tr.embed_weight.clone()
    g1, g2, num = e.backward_weights(out, cot, need_embed="update", embed_lr=0.25)
    assert (tr.w1._version, tr.w2._version) == versions and int(num) == int(sampled_rows(tr).sum())
    assert not torch.equal(old, tr.embed_weight)
    again = fresh()
    assert not torch.equal(again, after)
    assert torch.equal(served(), again), "a role pipeline does not see an update of the embedding alone"
    assert torch.equal(tr.embed(probe, 77), again)


def spread_graph():
    """The small graph with node v renamed 32 v among 2^18 nodes (the others have no edge), under the identity index: an index spread
    over embed_rows = 2^18 by a factor 32, in a form an indexed engine takes (it wants embed_rows <= num_nodes).  A dense gradient is
    2^18 x 64 floats = 64 MiB."""
    if "spread" not in _state:
        g = small_graph()["graph"]
        n = g.num_nodes * 32
        deg = np.zeros(n, dtype=np.int64)
        deg[::32] = np.diff(np.asarray(g.rowptr))
        rowptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
        col = (np.asarray(g.col).astype(np.int64) * 32).astype(np.int32)
        _state["spread"] = (torch.from_numpy(rowptr).to(DEV), torch.from_numpy(col).to(DEV), n)
    return _state["spread"]


def test_a_sparse_step_allocates_less_than_one_dense_gradient():
    rowptr, col, n = spread_graph()
    assert n == 1 << 18
    s = small_graph()
    index, rows = one_hot_index(n, DEV)
    dense_gradient = rows * EMBED_DIM * 4
    assert rows == 1 << 18 and dense_gradient == 64 << 20
    labels = torch.zeros(BATCH, dtype=torch.int64, device=DEV)
    rise = {}
    for sparse in (True, False):
        torch.manual_seed(5)
        tr = EngineTrainer(rowptr, col, None, 5, hidden1=32, hidden2=32, num_sample1=7, num_sample2=9, lr=0.3, max_batch=BATCH,
                           embed_index=index, embed_rows=rows, embed_dim=EMBED_DIM, sparse_embed=sparse)
        ids = [torch.from_numpy((s["cand"][i * BATCH:(i + 1) * BATCH] * 32).astype(np.int32)).to(DEV) for i in range(2)]
        tr.step(ids[0], labels, 1)                                              # warm-up: every scratch buffer exists
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        start = torch.cuda.memory_allocated()
        loss = tr.step(ids[1], labels, 2)
        torch.cuda.synchronize()
        rise[sparse] = torch.cuda.max_memory_allocated() - start
        assert bool(torch.isfinite(loss))
        del tr
    print(f"peak allocation above the start of a step: sparse {rise[True] / 2 ** 20:.2f} MiB, dense {rise[False] / 2 ** 20:.2f} MiB "
          f"(one dense gradient {dense_gradient / 2 ** 20:.0f} MiB)")
    assert rise[True] < dense_gradient, "a sparse step allocated as much as a dense gradient"
    assert rise[False] >= dense_gradient, "the dense step is expected to hold a dense gradient: the comparison would be vacuous"


def _cora():
    z = np.load(os.path.join(GOLDEN_DIR, "cora_topology.npz"))
    g = CSRGraph(z["rowptr"], z["col"], len(z["rowptr"]) - 1)
    _, labels = standin_citation(g, num_classes=7, feat_dim=64, seed=0)
    return g, labels


def test_a_node_embedding_trains_sparsely_on_the_cora_standin():
    g, labels = _cora()
    torch.manual_seed(0)
    res = run_engine_training(g, None, labels, 7, seed=1, epochs=5, batch_size=256, initializer="1hot", sparse_embed=True)
    losses, tr = res["losses"], res["trainer"]
    q = max(len(losses) // 4, 1)
    first, last = float(np.mean(losses[:q])), float(np.mean(losses[-q:]))
    print(f"1hot, sparse update, on stand-in Cora: {len(losses)} steps, mean loss {first:.4f} -> {last:.4f}, F1 micro {res['f1_micro']:.3f} "
          f"macro {res['f1_macro']:.3f}, {res['mean_step_time'] * 1e3:.3f} ms per step")
    assert tr.sparse_embed and np.all(np.isfinite(losses)) and last < first
    torch.manual_seed(0)
    rowptr, col = g.to(DEV)
    index, rows = one_hot_index(g.num_nodes, DEV)
    start = EngineTrainer(rowptr, col, None, 7, embed_index=index, embed_rows=rows, embed_dim=100, max_batch=256)
    assert tuple(tr.embed_weight.shape) == (g.num_nodes, 100)
    assert not torch.equal(start.embed_weight, tr.embed_weight), "the embedding has not moved"


def test_the_refusals():
    s = small_graph()
    index, rows = s["index"]["degree"]
    with pytest.raises(native.SageError, match="sparse_embed"):
        EngineTrainer(s["rowptr"], s["col"], torch.zeros(s["n"], 64, device=DEV), 5, sparse_embed=True)
    with pytest.raises(native.SageError, match="sparse_embed"):
        run_engine_training(s["graph"], np.zeros((s["n"], 8), dtype=np.float32), np.zeros(s["n"], dtype=np.int64), 5, sparse_embed=True)
    plain = TwoHopEngine(s["rowptr"], s["col"], torch.zeros(s["n"], 64, device=DEV), torch.zeros(32, 64, device=DEV),
                         torch.zeros(16, 32, device=DEV), 7, 9, max_batch=64)
    out = plain.forward(batch(0)[0][:64].contiguous(), seed=1)
    for form, lr in (("rows", None), ("update", 0.5)):
        with pytest.raises(native.SageError, match="need_embed"):
            plain.backward_weights(out, torch.zeros_like(out), need_embed=form, embed_lr=lr)
    tr = trainer("degree", True)
    out = tr.engine.forward(batch(0)[0], seed=1)
    with pytest.raises(native.SageError, match="embed_lr"):
        tr.engine.backward_weights(out, torch.zeros_like(out), need_embed="update")
