"""Node and degree embeddings on the sampled engine path (aggregators.py:68-71 under model.py:240-252's mini-batches): an indexed
TwoHopEngine against the plain engine on the materialised features, against the reference's own outputs and gradients, EngineTrainer's
four gradients against fp64 autograd on the sets the engine drew, reproducibility, training, serving through a RolePipeline, and the
refusals."""
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
from util import GOLDEN_DIR, assert_close_rowmax, load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda"
ACTS = {"relu": ops.ACT_RELU, "sigmoid": ops.ACT_SIGMOID}

_state = {}


def small_graph():
    """tests/test_gpu_engine_train.py's graph, its three indices and 1100 candidate seeds of non-zero degree, built once."""
    if not _state:
        graph = rmat_graph(13, 150_000, seed=4, accel=None)
        rowptr, col = graph.to(DEV)
        n = graph.num_nodes
        deg_idx, deg_rows = degree_index(rowptr)
        one_idx, one_rows = one_hot_index(n, DEV)
        _state.update(graph=graph, rowptr=rowptr, col=col, n=n,
                      index={"degree": (deg_idx, deg_rows), "identity": (one_idx, one_rows),
                             "zero": (torch.zeros(n, dtype=torch.int32, device=DEV), 1)},
                      cand=np.random.default_rng(2).choice(np.nonzero(graph.degrees() > 0)[0], 1100, replace=False))
    return _state


def live_sorted(eng):
    """The live layer-1 rows of the last forward, sorted by node id: (s1_nodes, cnt1, nbr1, h1)."""
    it = eng.intermediates()
    order = torch.argsort(it["s1_nodes"].long())
    return it["s1_nodes"][order], it["cnt1"][order], it["nbr1"][order], it["h1"][order]


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("act", sorted(ACTS))
@pytest.mark.parametrize("kind,batch", [("degree", 300), ("identity", 300), ("zero", 300), ("degree", 1024)])
def test_the_indexed_forward_is_the_plain_engine_on_the_materialised_features(kind, batch, act, fused):
    """embed + embed_index against X = embed[index] through the plain engine: the same outputs, sets and layer-1 state, bit for bit.
    1024 seeds x 9 outer samples reach the size at which layer 1 runs split (gather, then contraction) when fused."""
    s = small_graph()
    index, rows = s["index"][kind]
    gen = torch.Generator().manual_seed(7)
    embed = torch.randn(rows, 64, generator=gen).to(DEV)
    w1 = (torch.randn(32, 64, generator=gen) * 0.2).to(DEV)
    w2 = (torch.randn(16, 32, generator=gen) * 0.2).to(DEV)
    kw = dict(act1=ACTS[act], fused=fused, max_batch=batch, slice_major=False)
    indexed = TwoHopEngine(s["rowptr"], s["col"], embed, w1, w2, 7, 9, embed_index=index, **kw)
    plain = TwoHopEngine(s["rowptr"], s["col"], embed[index.long()].contiguous(), w1, w2, 7, 9, **kw)
    assert indexed.layout.layer1_split == plain.layout.layer1_split == int(fused and batch == 1024)
    assert indexed.layout.total_bytes == plain.layout.total_bytes and indexed.layout.max_s1 == plain.layout.max_s1
    assert indexed.table.data_ptr() == embed.data_ptr() and indexed._table_sliced is None
    seeds = torch.from_numpy(s["cand"][:batch].astype(np.int32)).to(DEV)
    for key in (11, 12):
        a, b = indexed.forward(seeds, seed=key), plain.forward(seeds, seed=key)
        assert torch.equal(a, b), f"{int((a != b).sum())} outputs differ"
        na, ca, ra, ha = live_sorted(indexed)
        nb, cb, rb, hb = live_sorted(plain)
        assert torch.equal(na, nb) and torch.equal(ca, cb) and len(na) > batch
        mask = torch.arange(7, device=DEV)[None, :] < ca[:, None]
        assert torch.equal(ra[mask], index[rb[mask].long()]), "nbr1 of the indexed engine is not embed_index of the plain engine's"
        assert torch.equal(ha, hb)


@pytest.mark.parametrize("name", ["tiny_1hot", "tiny_node_degree"])
def test_the_indexed_engine_matches_the_reference_outputs_and_gradients(name):
    """tests/golden/tiny_*.npz: the imported reference's enc2 output and its gradients of (W1, W2, embed) on injected sets.  The sets
    become CSR rows with k >= the longest row; the embedding and W1 are zero-padded from width 7 to 8."""
    from test_gpu_forward import csr_of_sets
    g = load_golden(name)
    n, rows = int(g["num_nodes"]), g["embed"].shape[0]
    rp1, c1 = csr_of_sets(g["layer1_nodes"], g["nbr1"], g["cnt1"], n)
    rp2, c2 = csr_of_sets(g["seeds"], g["nbr2"], g["cnt2"], n)
    index = np.zeros(n, dtype=np.int32)
    assert np.all(g["feat_rows"].sum(1) == 1) and g["feat_rows"].shape[1] == rows
    index[g["feat_ids"]] = g["feat_rows"].argmax(1)                 # the position of the one in each one-hot feature row
    embed = torch.zeros(rows, 8)
    embed[:, :7] = torch.from_numpy(g["embed"])
    w1 = torch.zeros(g["w1"].shape[0], 8)
    w1[:, :7] = torch.from_numpy(g["w1"])
    act1 = ops.ACT_SIGMOID if int(g["sigmoid1"]) else ops.ACT_RELU
    act2 = ops.ACT_SIGMOID if int(g["sigmoid2"]) else ops.ACT_RELU
    eng = TwoHopEngine(rp1, c1, embed.to(DEV), w1.to(DEV), torch.from_numpy(g["w2"]).to(DEV), k1=int(g["cnt1"].max()), k2=int(g["cnt2"].max()),
                       act1=act1, act2=act2, max_batch=len(g["seeds"]), rowptr_outer=rp2, col_outer=c2,
                       embed_index=torch.from_numpy(index).to(DEV))
    eng.keep_means = True
    out = eng.forward(torch.from_numpy(g["seeds"].astype(np.int32)).to(DEV), seed=1)
    assert_close_rowmax(out.cpu().t(), g["enc2_out"], rows_dim=1, what=f"{name} enc2_out")
    cot = torch.from_numpy(np.ascontiguousarray(g["cotangent"].T)).to(DEV)
    g_w1, g_w2, g_embed = eng.backward_weights(out, cot, need_embed=True)
    assert tuple(g_embed.shape) == (rows, 8) and not g_embed[:, 7].any(), "the padded column of g_embed is not exact zeros"
    for got, key in ((g_w1[:, :7], "grad_w1"), (g_w2, "grad_w2"), (g_embed[:, :7], "grad_embed")):
        err = ((got.double().cpu() - torch.from_numpy(g[key]).double()).abs().max() / np.abs(g[key]).max()).item()
        print(f"{name} {key}: max |got - golden| / max|golden| = {err:.2e}")
        assert err < 5e-5, f"{name} {key}: {err:.2e}"


def _autograd_reference(tr, seeds, labels):
    """tests/test_gpu_engine_train.py's fp64 reference with the table replaced by the embedding: nbr1 already holds embedding rows."""
    e = tr.engine
    it = e.intermediates()
    row2, cnt2 = it["row2"].cpu().long(), it["cnt2"].cpu().long()
    nbr1, cnt1 = it["nbr1"].cpu().long(), it["cnt1"].cpu().long()
    emb = tr.embed_weight.detach().cpu().double().requires_grad_(True)
    w1 = tr.w1.detach().cpu().double().requires_grad_(True)
    w2 = tr.w2.detach().cpu().double().requires_grad_(True)
    wc = tr.w_cls.detach().cpu().double().requires_grad_(True)

    def mean_rows(src, idx, cnt):
        m = (torch.arange(idx.shape[1])[None, :] < cnt[:, None]).double()
        return (src[idx.clamp_min(0)] * m[:, :, None]).sum(1) / cnt[:, None].double()

    act1 = torch.sigmoid if e.act1 == ops.ACT_SIGMOID else torch.relu
    h1 = act1(mean_rows(emb, nbr1, cnt1) @ w1.t())
    out = torch.relu(mean_rows(h1, row2, cnt2) @ w2.t())
    loss = torch.nn.functional.cross_entropy(out @ wc.t(), labels.cpu())
    used = torch.zeros(emb.shape[0], dtype=torch.bool)
    used[nbr1[torch.arange(nbr1.shape[1])[None, :] < cnt1[:, None]]] = True
    return loss.item(), torch.autograd.grad(loss, (w1, w2, wc, emb)), used


@pytest.mark.parametrize("embed_dim,hidden1", [(64, 32), (52, 30)])
@pytest.mark.parametrize("act", sorted(ACTS))
@pytest.mark.parametrize("kind", ["degree", "identity", "zero"])
def test_embedding_trainer_gradients_match_fp64_autograd_on_the_same_sets(kind, act, embed_dim, hidden1):
    s = small_graph()
    index, rows = s["index"][kind]
    seeds_np = s["cand"][:300]
    seeds = torch.from_numpy(seeds_np.astype(np.int32)).to(DEV)
    labels = torch.from_numpy(np.random.default_rng(3).integers(0, 5, 300)).to(DEV)
    heads = ("torch", "native") if (kind, act, embed_dim) == ("degree", "sigmoid", 64) else ("torch",)
    for head in heads:
        torch.manual_seed(3)
        tr = EngineTrainer(s["rowptr"], s["col"], None, 5, hidden1=hidden1, hidden2=64, num_sample1=7, num_sample2=9, max_batch=300, head=head,
                           embed_index=index, embed_rows=rows, embed_dim=embed_dim, act1=ACTS[act])
        assert len(tr.parameters()) == 4 and tuple(tr.embed_weight.shape) == (rows, embed_dim)
        loss, grads = tr.grads(seeds, labels, key=11)
        assert len(grads) == 4
        ref_loss, ref, used = _autograd_reference(tr, seeds_np, labels)
        assert abs(loss.item() - ref_loss) <= 1e-5 * max(1.0, abs(ref_loss))
        for name, g, r in zip(("w1", "w2", "w_cls", "embed"), grads, ref):
            assert g.shape == r.shape
            err = (g.cpu().double() - r).abs().max().item() / r.abs().max().item()
            print(f"{kind} {act} {embed_dim}/{hidden1} head {head} grad {name}: max |g - ref| / max|ref| = {err:.2e}")
            assert err <= 2e-5, f"grad {name}: max |g - ref| / max|ref| = {err:.2e}"
        if kind != "zero":
            assert bool((~used).any())
        assert not grads[3].cpu()[~used].any(), "an embedding row that no sampled node points to must get exact zeros"
        # the weight gradients do not depend on whether the embedding's gradient is asked for
        e = tr.engine
        out = e.forward(seeds, seed=11)
        cot = torch.randn(out.shape, generator=torch.Generator().manual_seed(1)).to(DEV)
        g1, g2 = e.backward_weights(out, cot)
        h1, h2, he = e.backward_weights(out, cot, need_embed=True)
        assert torch.equal(g1, h1) and torch.equal(g2, h2) and tuple(he.shape) == (rows, embed_dim)


def test_two_embedding_trainers_from_one_seed_stay_bit_identical():
    s = small_graph()
    index, rows = s["index"]["degree"]
    labels_by_node = torch.from_numpy(np.random.default_rng(3).integers(0, 5, s["n"])).to(DEV)
    batches = [torch.from_numpy(s["cand"][i * 256:(i + 1) * 256].astype(np.int32)).to(DEV) for i in range(3)]

    def run():
        torch.manual_seed(5)
        tr = EngineTrainer(s["rowptr"], s["col"], None, 5, hidden1=32, hidden2=32, num_sample1=7, num_sample2=9, lr=0.3, max_batch=256,
                           embed_index=index, embed_rows=rows, embed_dim=64, act1=ops.ACT_SIGMOID)
        first = tr.embed_weight.clone()
        losses = [tr.step(b, labels_by_node[b.long()], 100 + i).clone() for i, b in enumerate(batches)]
        return tr, first, losses

    a, first_a, la = run()
    b, first_b, lb = run()
    assert torch.equal(first_a, first_b) and not torch.equal(first_a, a.embed_weight)
    for x, y in zip(la, lb):
        assert torch.equal(x, y) and bool(torch.isfinite(x))
    for name, x, y in zip(("w1", "w2", "w_cls", "embed_weight"), a.parameters(), b.parameters()):
        assert torch.equal(x, y), f"{name}: two runs differ at {int((x != y).sum())} elements"
    # the three weights start as the frozen trainer's do for the same torch seed: the embedding is drawn after them
    torch.manual_seed(5)
    frozen = EngineTrainer(s["rowptr"], s["col"], torch.zeros(s["n"], 64, device=DEV), 5, hidden1=32, hidden2=32, num_sample1=7, num_sample2=9,
                           max_batch=256)
    torch.manual_seed(5)
    fresh = EngineTrainer(s["rowptr"], s["col"], None, 5, hidden1=32, hidden2=32, num_sample1=7, num_sample2=9, max_batch=256,
                          embed_index=index, embed_rows=rows, embed_dim=64)
    for x, y in zip(frozen.parameters(), fresh.parameters()[:3]):
        assert torch.equal(x, y)


def _cora():
    z = np.load(os.path.join(GOLDEN_DIR, "cora_topology.npz"))
    g = CSRGraph(z["rowptr"], z["col"], len(z["rowptr"]) - 1)
    _, labels = standin_citation(g, num_classes=7, feat_dim=64, seed=0)
    return g, labels


def test_a_node_embedding_trains_on_the_cora_standin():
    g, labels = _cora()
    torch.manual_seed(0)
    res = run_engine_training(g, None, labels, 7, seed=1, epochs=5, batch_size=256, initializer="1hot")
    losses, tr = res["losses"], res["trainer"]
    q = max(len(losses) // 4, 1)
    first, last = float(np.mean(losses[:q])), float(np.mean(losses[-q:]))
    print(f"1hot on stand-in Cora: {len(losses)} steps, mean loss {first:.4f} -> {last:.4f}, F1 micro {res['f1_micro']:.3f} macro "
          f"{res['f1_macro']:.3f}, {res['mean_step_time'] * 1e3:.3f} ms per step")
    assert np.all(np.isfinite(losses)) and last < first
    torch.manual_seed(0)
    rowptr, col = g.to(DEV)
    index, rows = one_hot_index(g.num_nodes, DEV)
    start = EngineTrainer(rowptr, col, None, 7, embed_index=index, embed_rows=rows, embed_dim=100, max_batch=256)
    assert tuple(tr.embed_weight.shape) == (g.num_nodes, 100)
    assert not torch.equal(start.embed_weight, tr.embed_weight), "the embedding has not moved"
    # rows of nodes that were never sampled are untouched, bit for bit: two small steps, the sampled rows read back after each
    before = start.embed_weight.clone()
    touched = torch.zeros(rows, dtype=torch.bool, device=DEV)
    labels_dev = torch.from_numpy(np.asarray(labels).reshape(-1)).to(DEV)
    for i in range(2):
        ids = torch.arange(64 * i, 64 * (i + 1), dtype=torch.int32, device=DEV)
        start.step(ids, labels_dev[ids.long()], key=i)
        it = start.engine.intermediates()
        mask = torch.arange(it["nbr1"].shape[1], device=DEV)[None, :] < it["cnt1"][:, None]
        touched[it["nbr1"][mask].long()] = True
    assert bool(touched.any()) and bool((~touched).any())
    assert torch.equal(start.embed_weight[~touched], before[~touched]), "a row nobody sampled was written"
    assert not torch.equal(start.embed_weight[touched], before[touched])


def test_a_degree_embedding_trains_for_an_epoch_and_predicts():
    g, labels = _cora()
    for head in ("torch", "native"):
        torch.manual_seed(0)
        res = run_engine_training(g, None, labels, 7, seed=1, epochs=1, batch_size=256, initializer="node_degree", head=head)
        tr = res["trainer"]
        print(f"node_degree on stand-in Cora, head {head}: F1 micro {res['f1_micro']:.3f} macro {res['f1_macro']:.3f}")
        assert np.all(np.isfinite(res["losses"])) and tr.engine.act1 == ops.ACT_SIGMOID
        assert tr.embed_weight.shape[0] == int(g.degrees().max()) + 1
        ids = torch.arange(200, dtype=torch.int32, device=DEV)
        pred = tr.predict(ids, key=3)
        assert pred.shape == (200,) and int(pred.min()) >= 0 and int(pred.max()) < 7
        assert tuple(tr.scores(ids, key=3).shape) == (200, 7) and tuple(tr.embed(ids, key=3).shape) == (200, 128)


def test_a_role_pipeline_serves_the_indexed_engine_and_sees_embedding_updates():
    s = small_graph()
    index, rows = s["index"]["degree"]
    gen = torch.Generator().manual_seed(9)
    embed = torch.randn(rows, 64, generator=gen).to(DEV)
    w1 = (torch.randn(32, 64, generator=gen) * 0.2).to(DEV)
    w2 = (torch.randn(16, 32, generator=gen) * 0.2).to(DEV)
    b = 256
    eng = TwoHopEngine(s["rowptr"], s["col"], embed, w1, w2, 7, 9, max_batch=b, embed_index=index)
    pipe = RolePipeline(s["rowptr"], s["col"], embed, w1, w2, 7, 9, batch=b, depth=2, embed_index=index)
    assert all(e.embed_index is index and e._col1_model is pipe.engines[0]._col1_model for e in pipe.engines)
    batches = [torch.from_numpy(s["cand"][i * b:(i + 1) * b].astype(np.int32)).to(DEV) for i in range(3)]

    def serve(keys):
        outs = torch.zeros(3, b, 16, device=DEV)
        for i, (ids, key) in enumerate(zip(batches, keys)):
            pipe.submit(ids, key, outs[i])
        pipe.synchronize()
        return outs

    def check(keys, what):
        outs = serve(keys)
        for i, (ids, key) in enumerate(zip(batches, keys)):
            assert torch.equal(outs[i], eng.forward(ids, seed=key)), f"{what}: batch {i} differs from the engine"
        return outs

    before = check((21, 22, 23), "before the update")
    with torch.no_grad():
        embed.add_(torch.randn(rows, 64, generator=gen).to(DEV), alpha=0.5)       # an SGD step's write, in place
    pipe.refresh_weights()
    pipe.fork()
    after = check((21, 22, 23), "after the update")
    assert not torch.equal(before, after)


def test_the_refusals():
    s = small_graph()
    index, rows = s["index"]["degree"]
    rowptr, col, n = s["rowptr"], s["col"], s["n"]
    embed = torch.zeros(rows, 64, device=DEV)
    w1, w2 = torch.zeros(32, 64, device=DEV), torch.zeros(16, 32, device=DEV)
    with pytest.raises(native.SageError, match="concat"):
        TwoHopEngine(rowptr, col, embed, torch.zeros(32, 128, device=DEV), torch.zeros(16, 64, device=DEV), 7, 9, concat=True, embed_index=index)
    with pytest.raises(native.SageError, match="self loop"):
        TwoHopEngine(rowptr, col, embed, w1, w2, 7, 9, agg_self_loop=True, embed_index=index)
    with pytest.raises(native.SageError, match="relabel"):
        TwoHopEngine(rowptr, col, embed, w1, w2, 7, 9, relabel="degree", embed_index=index)
    with pytest.raises(native.SageError, match="multiple of 4"):
        TwoHopEngine(rowptr, col, torch.zeros(rows, 50, device=DEV), torch.zeros(32, 50, device=DEV), w2, 7, 9, embed_index=index)
    with pytest.raises(native.SageError, match="outside"):
        TwoHopEngine(rowptr, col, embed[:rows - 1], w1, w2, 7, 9, embed_index=index)               # an index value at R
    with pytest.raises(native.SageError, match="R = "):
        TwoHopEngine(rowptr, col, torch.zeros(n + 1, 64, device=DEV), w1, w2, 7, 9, embed_index=index)
    tr = EngineTrainer(rowptr, col, None, 5, hidden1=32, hidden2=32, num_sample1=7, num_sample2=9, max_batch=64, embed_index=index,
                       embed_rows=rows, embed_dim=64)
    ring = torch.from_numpy(s["cand"][:128].astype(np.int32).reshape(2, 64)).to(DEV)
    with pytest.raises(native.SageError, match="capture_step"):
        tr.capture_step(ring, [1, 2], torch.zeros(n, dtype=torch.int64, device=DEV))
    plain = TwoHopEngine(rowptr, col, torch.zeros(n, 64, device=DEV), w1, w2, 7, 9, max_batch=64)
    out = plain.forward(ring[0], seed=1)
    with pytest.raises(native.SageError, match="need_embed"):
        plain.backward_weights(out, torch.zeros_like(out), need_embed=True)
