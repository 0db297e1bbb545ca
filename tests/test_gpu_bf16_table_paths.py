"""A feature table STORED as bf16 through the users of the full-neighbourhood mean: whole-graph and seed-batch inference, the exact
mini-batch trainer and the whole-graph trainer.  bf16 is a storage format only -- the mean widens each element exactly -- so the oracle
is exact: with T16 = table.to(torch.bfloat16), every result is bit for bit what the same call gives on T16.float().  Also here: the
paths that have no bf16 form refuse one by name, and a seed-batch call on a bf16 table allocates nothing of the table's fp32 size."""
import numpy as np
import pytest
import torch
import torch.nn as nn

from sage355 import native, ops
from sage355.datasets import standin_citation
from sage355.exactbatch import ExactBatchTrainer, run_exact_batch_training
from sage355.fullgraph import FullGraphTrainer, run_full_graph_training
from sage355.graph import CSRGraph, rmat_graph
from sage355.inference import embed_all_from_modules, embed_all_nodes, embed_nodes, embed_nodes_from_modules, layer_all_nodes

pytestmark = pytest.mark.gpu
DEV = "cuda"
E = native.CSR_MEAN_CHUNK
CLASSES, TRAIN = 5, 300


def bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def skewed_graph(seed=0):
    """tests/test_gpu_csr_mean.py's generator (degrees 0, 1, E-1, E, E+1, 2E, 2E+1, a hub of 20E + 37, self entries)."""
    rng = np.random.default_rng(seed)
    n = 24 * E
    special = {0: 0, 1: 1, 2: E - 1, 3: E, 4: E + 1, 5: 2 * E, 6: 2 * E + 1, 7: 20 * E + 37, 8: E + 1, 9: 2 * E + 1}
    deg = rng.integers(0, 7, n)
    for v, d in special.items():
        deg[v] = d
    rowptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(deg, out=rowptr[1:])
    col = rng.integers(0, n, int(rowptr[-1])).astype(np.int32)
    col[rowptr[7]:rowptr[8]] = rng.permutation(n)[: deg[7]]
    for v in (3, 8, 9, 20, 21, 22):
        if deg[v] > 0:
            col[rowptr[v + 1] - 1] = v
    col[rowptr[7] + 5 * E + 3] = 7
    return rowptr, col


@pytest.fixture(scope="module")
def sym():
    """skewed_graph symmetrised (every edge in both directions, stored order kept per row): 12,288 nodes, rows far past one chunk."""
    rowptr, col = skewed_graph()
    n = len(rowptr) - 1
    src = np.repeat(np.arange(n), np.diff(rowptr))
    s = np.concatenate([src, col.astype(np.int64)])
    d = np.concatenate([col.astype(np.int64), src])
    order = np.argsort(s, kind="stable")
    rp = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(s, minlength=n), out=rp[1:])
    assert int(np.diff(rp).max()) > 20 * E
    return torch.from_numpy(rp).to(DEV), torch.from_numpy(d[order].astype(np.int32)).to(DEV), n


def weights(d0, h1, h2, concat, seed):
    gen = torch.Generator().manual_seed(seed)
    m = 2 if concat else 1
    return ((torch.randn(h1, m * d0, generator=gen) / (m * d0) ** 0.5).to(DEV), (torch.randn(h2, m * h1, generator=gen) / (m * h1) ** 0.5).to(DEV))


# ------------------------------------------------------------------------------------------------------------------- inference
@pytest.mark.parametrize("d0", [64, 50])
@pytest.mark.parametrize("concat", [False, True])
def test_inference_obeys_the_bit_rule(sym, concat, d0):
    """rows_per_call = 5000 < N: three blocks per layer, the last one short."""
    rp, cl, n = sym
    t16 = torch.randn(n, d0, generator=torch.Generator().manual_seed(d0)).to(DEV).to(torch.bfloat16)
    t32 = t16.float()
    w1, w2 = weights(d0, 48, 40, concat, d0)
    kw = dict(concat=concat, agg_self_loop=not concat, rows_per_call=5000)
    h16 = layer_all_nodes(rp, cl, t16, w1, concat, not concat, ops.ACT_RELU, rows_per_call=5000)
    assert bits_equal(h16, layer_all_nodes(rp, cl, t32, w1, concat, not concat, ops.ACT_RELU, rows_per_call=5000)), "layer_all_nodes"
    all16 = embed_all_nodes(rp, cl, t16, w1, w2, **kw)
    assert all16.dtype == torch.float32 and bits_equal(all16, embed_all_nodes(rp, cl, t32, w1, w2, **kw)), "embed_all_nodes"
    rng = np.random.default_rng(d0)
    seeds = np.concatenate([np.arange(12), [7, 7, 0], rng.integers(0, n, 300)]).astype(np.int32)
    some16 = embed_nodes(rp, cl, t16, w1, w2, seeds, **dict(kw, rows_per_call=700))       # the frontier splits into blocks as well
    assert bits_equal(some16, embed_nodes(rp, cl, t32, w1, w2, seeds, **dict(kw, rows_per_call=700))), "embed_nodes"
    assert bits_equal(some16, all16[torch.from_numpy(seeds.astype(np.int64)).to(DEV)]), "embed_nodes(seeds) != embed_all_nodes()[seeds]"
    index = torch.arange(n, dtype=torch.int32, device=DEV)
    for call in (lambda: embed_all_nodes(rp, cl, t16, w1, w2, index=index, **kw), lambda: embed_nodes(rp, cl, t16, w1, w2, seeds, index=index, **kw),
                 lambda: layer_all_nodes(rp, cl, t16, w1, concat, False, ops.ACT_RELU, index=index)):
        with pytest.raises(native.SageError, match="bfloat16"):
            call()


def two_layer_modules(table, adj_lists, gcn, initializer="None"):
    from sage355.aggregators import MeanAggregator
    from sage355.encoders import Encoder
    features = nn.Embedding(*table.shape)
    features.weight = nn.Parameter(table.to(DEV), requires_grad=False)
    agg1 = MeanAggregator(features, cuda=True, gcn=gcn)
    enc1 = Encoder(features, table.shape[1], 24, adj_lists, agg1, num_sample=5, gcn=gcn, cuda=True, initializer=initializer)
    agg2 = MeanAggregator(lambda nodes: enc1(nodes).t(), cuda=True, gcn=gcn)
    return Encoder(lambda nodes: enc1(nodes).t(), enc1.embed_dim, 16, adj_lists, agg2, num_sample=5, base_model=enc1, gcn=gcn, cuda=True)


@pytest.fixture(scope="module")
def small():
    graph = rmat_graph(8, 1500, seed=2, accel=None)
    adj = {v: set(graph.neighbors(v).tolist()) for v in range(graph.num_nodes)}
    return graph, adj


@pytest.mark.parametrize("gcn", [True, False])
def test_the_module_entry_points_round_the_table_once(small, gcn):
    graph, adj = small
    table = torch.randn(graph.num_nodes, 20, generator=torch.Generator().manual_seed(1))
    torch.manual_seed(5)
    enc2 = two_layer_modules(table.clone(), adj, gcn)
    enc1 = enc2.base_model
    rp, cl = graph.to(DEV)
    t16 = table.to(DEV).to(torch.bfloat16)
    kw = dict(concat=not gcn, agg_self_loop=gcn)
    w1, w2 = enc1.weight.detach().to(DEV), enc2.weight.detach().to(DEV)
    got = embed_all_from_modules(enc2, table_dtype=torch.bfloat16)
    assert bits_equal(got, embed_all_nodes(rp, cl, t16, w1, w2, **kw))
    assert not bits_equal(got, embed_all_from_modules(enc2)), "the default reads the fp32 table"
    nodes = [3, 0, 200, 3, 17]
    assert bits_equal(embed_nodes_from_modules(enc2, nodes, table_dtype=torch.bfloat16), got[torch.tensor(nodes, device=DEV)])
    with pytest.raises(native.SageError):
        embed_all_from_modules(enc2, table_dtype=torch.float16)


# -------------------------------------------------------------------------------------------------------------------- trainers
@pytest.fixture(scope="module")
def setup():
    """tests/test_gpu_exact_batch_train.py's: 2048 nodes, a hub of 768 entries, isolated nodes among the seeds."""
    graph = rmat_graph(11, 30_000, seed=4, accel=None)
    deg = graph.degrees()
    assert graph.num_nodes == 2048 and int(deg.max()) > E and int((deg == 0).sum()) > 0
    rs = np.random.default_rng(2)
    ids = rs.choice(graph.num_nodes, TRAIN, replace=False)
    labels = torch.from_numpy(rs.integers(0, CLASSES, TRAIN))
    rowptr, col = graph.to(DEV)
    return graph, rowptr, col, torch.from_numpy(ids.astype(np.int32)).to(DEV), labels.to(DEV)


def another_association(g, ref):
    """tests/test_gpu_exact_batch_train.py's measure for "the same sums in another association": max |g - ref| / max |ref|, bar 2e-5."""
    return (g.cpu().double() - ref.cpu().double()).abs().max().item() / ref.cpu().double().abs().max().item()


@pytest.mark.parametrize("self_loop", [False, True])
@pytest.mark.parametrize("d0,h1", [(64, 32), (50, 30)])
@pytest.mark.parametrize("gcn", [True, False])
def test_exact_batch_trainer_obeys_the_bit_rule(setup, gcn, d0, h1, self_loop):
    graph, rowptr, col, seeds, tgt = setup
    t16 = torch.randn(graph.num_nodes, d0, generator=torch.Generator().manual_seed(d0)).to(DEV).to(torch.bfloat16)
    kw = dict(hidden1=h1, hidden2=64, gcn=gcn, agg_self_loop=self_loop)
    torch.manual_seed(3)
    a = ExactBatchTrainer(rowptr, col, t16, CLASSES, **kw)
    torch.manual_seed(3)
    b = ExactBatchTrainer(rowptr, col, t16.float(), CLASSES, **kw)
    assert a.table.dtype == torch.bfloat16
    for x, y in zip(a.parameters(), b.parameters()):
        assert bits_equal(x, y)
    assert bits_equal(a.forward(seeds), b.forward(seeds)), "forward"
    (la, ga), (lb, gb) = a.grads(seeds, tgt), b.grads(seeds, tgt)
    assert bits_equal(la.reshape(1), lb.reshape(1)), (la.item(), lb.item())
    assert bits_equal(ga[2], gb[2]), "g_cls"
    for name, x, y in (("g_w1", ga[0], gb[0]), ("g_w2", ga[1], gb[1])):
        err = another_association(x, y)
        print(f"{name}: gcn={gcn} bits equal {bits_equal(x, y)}, max |g - ref| / max |ref| = {err:.2e}")
        assert err <= 2e-5, f"{name}: {err:.2e}"
        # the own rows reach the contraction in the same order with the same values, widened or through the index: the same sums
        assert bits_equal(x, y), name
    assert bool((a.frontier.pos == -1).all())


@pytest.mark.parametrize("self_loop", [False, True])
@pytest.mark.parametrize("d0,h1", [(64, 32), (50, 30)])
def test_full_graph_trainer_obeys_the_bit_rule_with_gcn(setup, d0, h1, self_loop):
    graph, rowptr, col, seeds, tgt = setup
    t16 = torch.randn(graph.num_nodes, d0, generator=torch.Generator().manual_seed(d0)).to(DEV).to(torch.bfloat16)
    kw = dict(hidden1=h1, hidden2=64, gcn=True, agg_self_loop=self_loop)
    torch.manual_seed(3)
    a = FullGraphTrainer(rowptr, col, t16, CLASSES, **kw)
    torch.manual_seed(3)
    b = FullGraphTrainer(rowptr, col, t16.float(), CLASSES, **kw)
    assert bits_equal(a.forward(), b.forward()), "forward"
    (la, ga), (lb, gb) = a.grads(seeds, tgt), b.grads(seeds, tgt)
    assert bits_equal(la.reshape(1), lb.reshape(1))
    for name, x, y in zip(("g_w1", "g_w2", "g_cls"), ga, gb):
        assert bits_equal(x, y), name
    assert bits_equal(a.refresh_table(), b.refresh_table())
    with pytest.raises(native.SageError, match="bfloat16"):
        FullGraphTrainer(rowptr, col, t16, CLASSES, **dict(kw, gcn=False))


def test_twenty_exact_batch_steps_on_standin_citation_give_the_fp32_losses(setup):
    """Bag-of-words features are 0 / 1, exact in bf16: storing the table as bf16 changes no bit of the training run."""
    graph = setup[0]
    feats, labels = standin_citation(graph, num_classes=7, feat_dim=1433, seed=0)
    runs = {}
    for dtype in (torch.float32, torch.bfloat16):
        torch.manual_seed(0)
        res = run_exact_batch_training(graph, feats, labels, 7, seed=1, epochs=2, batch_size=128, table_dtype=dtype)
        assert res["trainer"].table.dtype == dtype
        runs[dtype] = torch.stack([torch.as_tensor(x).reshape(()).float().cpu() for x in res["losses"][:20]])
    assert runs[torch.float32].numel() == 20 and bool(torch.isfinite(runs[torch.float32]).all())
    assert bits_equal(runs[torch.bfloat16], runs[torch.float32]), (runs[torch.bfloat16].tolist(), runs[torch.float32].tolist())
    torch.manual_seed(0)
    res = run_full_graph_training(graph, feats, labels, 7, seed=1, steps=2, table_dtype=torch.bfloat16)
    assert res["trainer"].table.dtype == torch.bfloat16 and len(res["losses"]) == 2


# -------------------------------------------------------------------------------------------------------------------- refusals
def test_every_path_without_a_bf16_form_refuses_by_name(setup, small):
    from sage355.engine import RolePipeline, TwoHopEngine
    from sage355.train import EngineTrainer
    graph, rowptr, col, seeds, tgt = setup
    n = graph.num_nodes
    t16 = torch.zeros(n, 16, dtype=torch.bfloat16, device=DEV)
    w1, w2 = weights(16, 16, 16, False, 0)
    idx = torch.arange(n, dtype=torch.int32, device=DEV)
    embed = dict(embed_index=idx, embed_rows=n, embed_dim=16)
    calls = {
        "TwoHopEngine": lambda: TwoHopEngine(rowptr, col, t16, w1, w2, 5, 5),
        "RolePipeline": lambda: RolePipeline(rowptr, col, t16, w1, w2, 5, 5, batch=64),
        "EngineTrainer": lambda: EngineTrainer(rowptr, col, t16, CLASSES, hidden1=16, hidden2=16),
        "EngineTrainer(embed_index)": lambda: EngineTrainer(rowptr, col, t16, CLASSES, hidden1=16, hidden2=16, **embed),
        "FullGraphTrainer(embed_index)": lambda: FullGraphTrainer(rowptr, col, t16, CLASSES, hidden1=16, hidden2=16, **embed),
        "FullGraphTrainer(concat)": lambda: FullGraphTrainer(rowptr, col, t16, CLASSES, hidden1=16, hidden2=16, gcn=False),
        "run_exact_batch_training(1hot)": lambda: run_exact_batch_training(graph, None, np.zeros(n, dtype=np.int64), CLASSES, initializer="1hot",
                                                                           table_dtype=torch.bfloat16),
        "run_full_graph_training(node_degree)": lambda: run_full_graph_training(graph, None, np.zeros(n, dtype=np.int64), CLASSES,
                                                                                initializer="node_degree", table_dtype=torch.bfloat16),
        "csr_mean(index)": lambda: ops.csr_mean(rowptr, col, t16, index=idx),
    }
    for name, call in calls.items():
        with pytest.raises(native.SageError, match="bfloat16"):
            call()
    # the modules on the device path: a bf16 nn.Embedding feature table, two-layer stack and single layer, and an aggregator on its own
    small_graph, adj = small
    tab = torch.zeros(small_graph.num_nodes, 20, dtype=torch.bfloat16)
    for gcn in (True, False):
        enc2 = two_layer_modules(tab.clone(), adj, gcn)
        with pytest.raises(native.SageError, match="bfloat16"):
            enc2([0, 1, 2])
        with pytest.raises(native.SageError, match="bfloat16"):
            enc2.base_model([0, 1, 2])
        with pytest.raises(native.SageError, match="bfloat16"):
            enc2.base_model.aggregator([0, 1], [adj[0] | {5}, adj[1] | {6}], 5)


# ---------------------------------------------------------------------------------------------------------------------- memory
def test_embed_nodes_on_a_bf16_table_allocates_nothing_of_the_tables_fp32_size():
    """tests/test_gpu_exact_batch_train.py's pattern: 2^18 nodes, nearly all isolated, 64 seeds, the CONCAT encoder (the one form that
    widens table rows).  What a call may allocate: the frontier's [N] int32 map, and arrays with one row per frontier node -- the block
    of means and the widened own rows ([|F|, max(d0, h1)] fp32 each, and the bf16 rows they are widened from), h1_F, the outputs, the
    csr_mean workspace, the frontier's own lists and the integer temporaries that size them (a few 8-byte values per frontier node or
    seed edge).  Nothing in that has N * d0 elements: the bound below is far under ONE [N, d0] fp32 array, which an [N, d0] widening
    of the table would alone exceed."""
    n, d0, h1, h2, live = 1 << 18, 64, 32, 16, 4096
    rng = np.random.default_rng(0)
    deg = np.zeros(n, dtype=np.int64)
    deg[:live] = rng.integers(1, 9, live)
    rowptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(deg, out=rowptr[1:])
    col = rng.integers(0, live, int(rowptr[-1])).astype(np.int32)
    rp, cl = CSRGraph(rowptr, col, n).to(DEV)
    t16 = torch.randn(n, d0, device=DEV).to(torch.bfloat16)
    w1, w2 = weights(d0, h1, h2, True, 0)
    seeds_np = np.concatenate([rng.choice(live, 60, replace=False), live + np.arange(4)])
    seeds = torch.from_numpy(seeds_np.astype(np.int32)).to(DEV)
    frontier = np.unique(np.concatenate([seeds_np] + [col[rowptr[v]:rowptr[v + 1]] for v in seeds_np]))
    f, m = len(frontier), len(seeds_np)
    e2 = int(deg[seeds_np].sum())
    e1 = int(deg[frontier].sum())
    wide = max(d0, h1)
    bound = (4 * n                                                     # the map
             + 4 * f * (2 * wide + h1) + 2 * f * d0 + 4 * m * h2      # means, own rows (fp32 and bf16), h1_F, out
             + max(ops.csr_mean_workspace_bytes(f, e1, d0), ops.csr_mean_workspace_bytes(m, e2, h1))
             + 64 * (f + m + e2)                                      # the frontier's lists and the integer temporaries
             + (1 << 20))                                             # the allocator's rounding of every block above
    assert bound < 4 * n * d0 // 8, "the shapes must keep the bound far below one [N, d0] fp32 array"
    embed_nodes(rp, cl, t16, w1, w2, seeds, concat=True)                # warm-up: kernels loaded
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = embed_nodes(rp, cl, t16, w1, w2, seeds, concat=True)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated()
    print(f"|F| = {f}, allocated before {before}, peak above it {peak - before}, bound {bound}, one [N, d0] fp32 array {4 * n * d0}")
    assert bits_equal(out, embed_nodes(rp, cl, t16.float(), w1, w2, seeds, concat=True))
    assert peak - before <= bound, f"the call allocated {peak - before} bytes, more than {bound}"
