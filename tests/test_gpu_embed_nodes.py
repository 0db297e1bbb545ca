"""inference.embed_nodes on the MI355X: exact embeddings of a seed batch, bit for bit the rows of embed_all_nodes, in memory that
follows the frontier and not the graph; the module entry point, EngineTrainer.predict_exact and run_engine_training(exact_eval=True)."""
import math
import os

import numpy as np
import pytest
import torch

from sage355 import native, ops
from sage355.datasets import standin_citation
from sage355.graph import CSRGraph, csr_from_adj_lists, rmat_graph
from sage355.inference import embed_all_from_modules, embed_all_nodes, embed_nodes, embed_nodes_from_modules
from sage355.train import EngineTrainer, run_engine_training
from test_gpu_csr_frontier import HUB, ISOLATED, N, build_graph
from test_gpu_forward import build_modules
from util import GOLDEN_DIR, TWO_LAYER_CASES, assert_close_rowmax, full_table, load_golden, sets_from_padded

pytestmark = pytest.mark.gpu
D0, H1, H2 = 12, 10, 6
# the hub (so F is every node), the isolated node, duplicates, rows at the edges of the chunk split, rows of the contended pool
SEEDS_HUB = [HUB, ISOLATED, 33, 7, 7, 250, 9, 3, HUB, 8, 4000, 1, 2, 300, 33]
SEEDS_FEW = [33, ISOLATED, 7, 250, 250, 9, 3, 20, 21, 22, 301, 4095]


def bits_equal(a, b):
    """Bitwise equality, NaNs included (torch.equal says NaN != NaN)."""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def to_dev(rowptr, col):
    return torch.from_numpy(rowptr).cuda(), torch.from_numpy(col).cuda()


@pytest.fixture(scope="module")
def data():
    gen = torch.Generator().manual_seed(11)
    inner, outer = to_dev(*build_graph(0)), to_dev(*build_graph(1))
    table = torch.randn(N, D0, generator=gen).cuda()
    w = {False: (torch.randn(H1, D0, generator=gen).cuda() / 3, torch.randn(H2, H1, generator=gen).cuda() / 3),
         True: (torch.randn(H1, 2 * D0, generator=gen).cuda() / 4, torch.randn(H2, 2 * H1, generator=gen).cuda() / 4)}
    return inner, outer, table, w


def ids(seeds):
    return torch.tensor(seeds, dtype=torch.int64, device="cuda")


@pytest.mark.parametrize("sigmoid", [False, True])
@pytest.mark.parametrize("self_loop", [False, True])
@pytest.mark.parametrize("concat", [False, True])
def test_embed_nodes_has_the_bits_of_embed_all_nodes(data, concat, self_loop, sigmoid):
    (rp, cl), _, table, w = data
    act = ops.ACT_SIGMOID if sigmoid else ops.ACT_RELU
    kw = dict(concat=concat, agg_self_loop=self_loop, act1=act, act2=act)
    full = embed_all_nodes(rp, cl, table, *w[concat], **kw)
    assert torch.isnan(full[ISOLATED]).all() == (not self_loop)              # the isolated node is the NaN row (aggregators.py:60-61)
    for seeds, rows in ((SEEDS_HUB, 1 << 18), (SEEDS_HUB, 1000), (SEEDS_FEW, 1 << 18), (SEEDS_FEW, 7)):   # |F| = 4096 = 4 * 1000 + 96
        got = embed_nodes(rp, cl, table, *w[concat], seeds, rows_per_call=rows, **kw)
        assert got.shape == (len(seeds), H2)
        assert bits_equal(got, full[ids(seeds)]), (seeds[:3], rows)
    assert embed_nodes(rp, cl, table, *w[concat], [], **kw).shape == (0, H2)
    dev_seeds = torch.tensor(SEEDS_FEW, dtype=torch.int32, device="cuda")   # ids that are already on the device
    assert bits_equal(embed_nodes(rp, cl, table, *w[concat], dev_seeds, **kw), full[ids(SEEDS_FEW)])


@pytest.mark.parametrize("concat", [False, True])
def test_distinct_inner_and_outer_graphs(data, concat):
    (rp, cl), (rp2, cl2), table, w = data
    kw = dict(concat=concat, agg_self_loop=True, rowptr_outer=rp2, col_outer=cl2)
    full = embed_all_nodes(rp, cl, table, *w[concat], **kw)
    for seeds in (SEEDS_HUB, SEEDS_FEW):
        assert bits_equal(embed_nodes(rp, cl, table, *w[concat], seeds, rows_per_call=501, **kw), full[ids(seeds)])


@pytest.mark.parametrize("concat", [False, True])
def test_an_embedding_read_through_an_index(data, concat):
    """node_degree style: row min(degree, K - 1) of a [K, d0] embedding (aggregators.py:68-71)."""
    (rp, cl), _, _, w = data
    k = 40
    index = (rp[1:] - rp[:-1]).clamp(max=k - 1).to(torch.int32)
    embed = torch.randn(k, D0, generator=torch.Generator().manual_seed(5)).cuda()
    kw = dict(concat=concat, agg_self_loop=not concat, act1=ops.ACT_SIGMOID, index=index)
    full = embed_all_nodes(rp, cl, embed, *w[concat], **kw)
    for seeds in (SEEDS_HUB, SEEDS_FEW):
        assert bits_equal(embed_nodes(rp, cl, embed, *w[concat], seeds, rows_per_call=333, **kw), full[ids(seeds)])
    bad = index.clone()
    bad[5] = k
    with pytest.raises(native.SageError):
        embed_nodes(rp, cl, embed, *w[concat], SEEDS_FEW, **dict(kw, index=bad))


def test_two_calls_and_a_reused_frontier_give_the_same_bits(data):
    (rp, cl), _, table, w = data
    first = embed_nodes(rp, cl, table, *w[True], SEEDS_HUB, concat=True)
    assert bits_equal(embed_nodes(rp, cl, table, *w[True], SEEDS_HUB, concat=True), first)          # F's order may differ
    fr = ops.CsrFrontier(N, "cuda", max_nodes=0)
    for _ in range(2):
        assert bits_equal(embed_nodes(rp, cl, table, *w[True], SEEDS_HUB, concat=True, frontier=fr), first)
        assert fr.size() == 0 and bool((fr.pos == -1).all()), "the map was not cleared before returning"
    few = embed_nodes(rp, cl, table, *w[True], SEEDS_FEW, concat=True, frontier=fr)
    assert bits_equal(few, embed_nodes(rp, cl, table, *w[True], SEEDS_FEW, concat=True))


def test_bad_seeds_raise_and_leave_the_map_clean(data):
    (rp, cl), _, table, w = data
    fr = ops.CsrFrontier(N, "cuda", max_nodes=0)
    for bad in ([3, N], [-1, 3], torch.tensor([3, N], dtype=torch.int32, device="cuda"), torch.tensor([-5], dtype=torch.int32, device="cuda")):
        with pytest.raises(native.SageError):
            embed_nodes(rp, cl, table, *w[False], bad, frontier=fr)
    with pytest.raises(native.SageError):
        embed_nodes(rp, cl, table, *w[False], SEEDS_FEW, frontier=ops.CsrFrontier(N - 1, "cuda"))
    with pytest.raises(native.SageError):                                     # an error AFTER the frontier kernel ran: layer 1 refuses an int64 col
        embed_nodes(rp, cl.long(), table, *w[False], SEEDS_FEW, rowptr_outer=rp, col_outer=cl, frontier=fr)
    assert fr.max_nodes > 0, "the frontier kernel has not run"
    assert fr.size() == 0 and bool((fr.pos == -1).all())
    ops.csr_frontier(rp, cl, torch.tensor([HUB], dtype=torch.int32, device="cuda"), fr)          # a frontier that was not cleared
    with pytest.raises(native.SageError):
        embed_nodes(rp, cl, table, *w[False], SEEDS_FEW, frontier=fr)
    assert fr.size() == 0 and bool((fr.pos == -1).all()), "after an overflow the map is refilled"


@pytest.mark.parametrize("mode", ["gcn", "concat", "concat_index"])
@pytest.mark.parametrize("n,dim,out_dim", [(300, D0, H1), (97, H1, H2), (1000, 64, 50)])
def test_linear_act_bits_of_a_row_do_not_depend_on_its_position(n, dim, out_dim, mode):
    """The property that carries embed_nodes' bit contract: F comes in arbitrary order, and a row of embed_all_nodes sits at its node
    id.  Permute the rows of the input and compare; a shorter call gives the same rows too."""
    gen = torch.Generator().manual_seed(n)
    agg = torch.randn(n, dim, generator=gen).cuda()
    agg[5] = float("nan")
    tab = torch.randn(n + 9, dim, generator=gen).cuda()
    weight = (torch.randn(out_dim, dim * (1 if mode == "gcn" else 2), generator=gen) / 4).cuda()
    perm = torch.randperm(n, generator=gen).cuda()
    sidx = torch.randint(0, n + 9, (n,), generator=gen).to(torch.int32).cuda()
    for act in (ops.ACT_RELU, ops.ACT_SIGMOID):
        if mode == "gcn":
            base = ops.linear_act(agg, weight, act)
            moved = ops.linear_act(agg[perm].contiguous(), weight, act)
            short = ops.linear_act(agg[perm][: n // 3].contiguous(), weight, act)
        elif mode == "concat":
            base = ops.linear_act(agg, weight, act, self_tab=tab[:n])
            moved = ops.linear_act(agg[perm].contiguous(), weight, act, self_tab=tab[:n][perm].contiguous())
            short = ops.linear_act(agg[perm][: n // 3].contiguous(), weight, act, self_tab=tab, self_index=perm[: n // 3].to(torch.int32))
        else:
            base = ops.linear_act(agg, weight, act, self_tab=tab, self_index=sidx)
            moved = ops.linear_act(agg[perm].contiguous(), weight, act, self_tab=tab, self_index=sidx[perm].contiguous())
            short = ops.linear_act(agg[perm][: n // 3].contiguous(), weight, act, self_tab=tab, self_index=sidx[perm][: n // 3].contiguous())
        assert bits_equal(moved, base[perm]) and bits_equal(short, base[perm][: n // 3]), (mode, act)


def act_of(flag):
    return ops.ACT_SIGMOID if int(flag) else ops.ACT_RELU


@pytest.mark.parametrize("name", TWO_LAYER_CASES)
def test_embed_nodes_reproduces_reference_goldens(name):
    """Inner CSR = the fixture's layer-1 sets, outer CSR = its seeds' sets: embed_nodes on the fixture's seeds is the reference's enc2 output."""
    g = load_golden(name)
    table = full_table(g)
    n = table.shape[0]
    rp1, c1 = csr_from_adj_lists(sets_from_padded(g["layer1_nodes"], g["nbr1"], g["cnt1"]), num_nodes=n).to("cuda")
    rp2, c2 = csr_from_adj_lists(sets_from_padded(g["seeds"], g["nbr2"], g["cnt2"]), num_nodes=n).to("cuda")
    out = embed_nodes(rp1, c1, table.cuda(), torch.from_numpy(g["w1"]).cuda(), torch.from_numpy(g["w2"]).cuda(), g["seeds"].astype(np.int64),
                      concat=not bool(g["gcn"]), act1=act_of(g["sigmoid1"]), act2=act_of(g["sigmoid2"]), rowptr_outer=rp2, col_outer=c2,
                      rows_per_call=997)
    assert_close_rowmax(out.cpu().t(), g["enc2_out"], rows_dim=1, what=f"{name} enc2_out")


@pytest.mark.parametrize("name", ["tiny_sigmoid", "cora_emb_gcn_5_5", "cora_emb_concat_10_10"])
def test_embed_nodes_from_modules(name):
    g = load_golden(name)
    sets1 = sets_from_padded(g["layer1_nodes"], g["nbr1"], g["cnt1"])
    sets2 = sets_from_padded(g["seeds"], g["nbr2"], g["cnt2"])
    enc1, enc2 = build_modules(g, None, None, False, sets1, sets2)
    nodes = [int(s) for s in g["seeds"]] + [int(g["seeds"][0]), int(g["layer1_nodes"][-1])]
    emb = embed_nodes_from_modules(enc2, nodes)
    assert bits_equal(emb, embed_all_from_modules(enc2)[ids(nodes)])
    assert_close_rowmax(emb.cpu()[: len(g["seeds"])].t(), g["enc2_out"], rows_dim=1, what=f"{name} vs reference")


def test_embed_nodes_from_modules_refuses_what_embed_all_from_modules_refuses():
    g = load_golden("tiny_gcn")
    sets1 = sets_from_padded(g["layer1_nodes"], g["nbr1"], g["cnt1"])
    sets2 = sets_from_padded(g["seeds"], g["nbr2"], g["cnt2"])
    enc1, enc2 = build_modules(g, None, None, False, sets1, sets2)
    nodes = [int(s) for s in g["seeds"]]

    def refused(enc):
        for fn in (lambda: embed_nodes_from_modules(enc, nodes), lambda: embed_all_from_modules(enc)):
            with pytest.raises(native.SageError):
                fn()

    refused(enc1)                                              # no base model
    enc1.initializer = "node_degree"                           # ... whose aggregator was built without `embed`
    refused(enc2)
    enc1.initializer = "None"
    feats = enc1.features
    del enc1.features
    enc1.features = lambda i: feats(i)                         # not a feature table
    refused(enc2)
    del enc1.features
    enc1.features = feats
    agg = enc2.aggregator
    enc2.aggregator = torch.nn.Identity()                      # a foreign aggregator
    refused(enc2)
    enc2.aggregator = agg
    with pytest.raises(native.SageError):
        embed_nodes_from_modules(enc2, [0, enc1.features.weight.shape[0]])      # an id outside the graph
    assert embed_nodes_from_modules(enc2, nodes).shape == (len(nodes), enc2.weight.shape[0])


def test_memory_follows_the_frontier_not_the_graph():
    """A ring lattice of 2^18 nodes, degree 4, 8 seeds: the [N] map is 1 MB and |F| <= 40 rows, where one [N, h1] array is 64 MB."""
    n, d0, h = 1 << 18, 4, 64
    v = torch.arange(n, device="cuda")
    col = torch.stack([(v - 2) % n, (v - 1) % n, (v + 1) % n, (v + 2) % n], 1).reshape(-1).to(torch.int32)
    rowptr = torch.arange(n + 1, device="cuda") * 4
    gen = torch.Generator().manual_seed(2)
    table = torch.randn(n, d0, generator=gen).cuda()
    w1, w2 = torch.randn(h, d0, generator=gen).cuda() / 2, torch.randn(h, h, generator=gen).cuda() / 8
    seeds = torch.tensor([0, 1, 5, n - 1, 70_000, 70_003, 200_000, 131_072], dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = embed_nodes(rowptr, col, table, w1, w2, seeds)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    print(f"embed_nodes, 2^18-node ring, 8 seeds: peak {peak / 2 ** 20:.2f} MiB above the inputs")
    assert peak < 8 * 2 ** 20, peak
    # and the rows are right: against the layer written out with torch on the 40-node neighbourhood (fp64)
    t64, nb = table.double(), col.view(n, 4).long()
    h1 = torch.relu(t64[nb].mean(1) @ w1.double().t())
    ref = torch.relu(h1[nb[seeds.long()]].mean(1) @ w2.double().t())
    assert_close_rowmax(out.cpu(), ref.cpu(), what="ring lattice")


TRAINER_CASES = [(True, "torch", "degree", False), (False, "native", None, False), (True, "native", None, True)]


@pytest.mark.parametrize("gcn,head,relabel,embedding", TRAINER_CASES)
def test_predict_exact_is_the_heads_rule_on_embed_nodes(gcn, head, relabel, embedding):
    from sage355.fullgraph import degree_index
    graph = rmat_graph(12, 60_000, seed=1)
    rowptr, col = graph.to("cuda")
    n = graph.num_nodes
    torch.manual_seed(3)
    if embedding:
        index, rows = degree_index(rowptr)
        tr = EngineTrainer(rowptr, col, None, 4, hidden1=30, hidden2=16, num_sample1=5, num_sample2=5, gcn=gcn, max_batch=128, head=head,
                           embed_index=index, embed_rows=rows, embed_dim=8, act1=ops.ACT_SIGMOID)
        table = tr.embed_weight
    else:
        index, table = None, torch.randn(n, 66).cuda()
        tr = EngineTrainer(rowptr, col, table, 4, hidden1=30, hidden2=16, num_sample1=5, num_sample2=5, gcn=gcn, max_batch=128, head=head,
                           relabel=relabel)
    deg = graph.degrees()
    seeds = np.concatenate([[int(np.argmax(deg)), int(np.argmin(deg))], np.random.default_rng(0).choice(n, 198)]).astype(np.int32)
    dev_seeds = torch.from_numpy(seeds).cuda()
    labels = torch.from_numpy(np.random.default_rng(1).integers(0, 4, 128)).cuda()
    tr.step(dev_seeds[:128].contiguous(), labels, 7)                            # trained weights, not the initial ones
    emb = embed_nodes(rowptr, col, table, tr.w1, tr.w2, dev_seeds, concat=not gcn, act1=ops.ACT_SIGMOID if embedding else ops.ACT_RELU, index=index)
    assert bits_equal(tr.embed_exact(dev_seeds), emb)
    if head == "torch":
        want = (emb @ tr.w_cls.t()).argmax(1).to(torch.int32)
    else:
        want = ops.xent_head(emb, tr.w_cls, grads=False, pred=True)["pred"]
    pred = tr.predict_exact(dev_seeds)
    assert pred.dtype == torch.int32 and torch.equal(pred, want)
    assert torch.equal(tr.predict_exact(dev_seeds), pred) and torch.equal(tr.predict_exact(seeds.tolist()), pred)
    assert tr.predict(dev_seeds[:128].contiguous(), key=1).shape == tr.predict(dev_seeds[:128].contiguous(), key=2).shape   # sampled: may differ


@pytest.mark.parametrize("head", ["torch", "native"])
def test_exact_eval_leaves_training_untouched(head):
    z = np.load(os.path.join(GOLDEN_DIR, "cora_topology.npz"))
    g = CSRGraph(z["rowptr"], z["col"], len(z["rowptr"]) - 1)
    feats, labels = standin_citation(g, num_classes=7, feat_dim=1433, seed=0)
    res = {}
    for exact in (False, True):
        torch.manual_seed(0)
        res[exact] = run_engine_training(g, feats, labels, 7, seed=1, epochs=1, batch_size=256, head=head, exact_eval=exact)
    assert res[True]["losses"] == res[False]["losses"] and len(res[True]["losses"]) > 3
    for r in res.values():
        assert math.isfinite(r["f1_micro"]) and math.isfinite(r["f1_macro"]) and 0.0 <= r["f1_micro"] <= 1.0
    print(f"stand-in Cora, 1 epoch, head={head}: F1 micro sampled {res[False]['f1_micro']:.3f}, exact {res[True]['f1_micro']:.3f}")
