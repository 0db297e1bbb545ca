"""Round-3 GPU tests.  The execution path bench.py TIMES -- RolePipeline, depth 4, roles SGDL, engine-internal degree layout --
at BASELINE configs[2]'s full size, checked against the oracle WITHOUT the GPU's intermediates: the sampled sets are recomputed
by the C restatement of the sampler from (key, node id) alone, the frontier is their union, the values come from the fp64
restatement of aggregators.py:54-74 / encoders.py:49-62 on those sets."""
import os

import numpy as np
import pytest
import torch

from oracle import ref_sparse, sampler_ref
from sage355 import native as native_mod
from sage355 import ops
from sage355.engine import RolePipeline, TwoHopEngine
from sage355.graph import relabel_by_degree, rmat_graph
from util import assert_close_rowmax

pytestmark = pytest.mark.gpu
DEV = "cuda"
CACHE = os.environ.get("SAGE_CACHE", "/tmp/sage_cache")


def oracle_two_hop(graph, table, w1, w2, seeds, k1, k2, key, concat=False):
    """The whole 2-hop forward from (graph, seeds, key) alone: oracle/sampler_ref.c draws both hops, the frontier is the set
    union in any order (nothing computed from it depends on the order), oracle/ref_sparse.py does the arithmetic in fp64."""
    nbr2, cnt2 = sampler_ref.sample_neighbors(graph.rowptr, graph.col, seeds, k2, key, ops.TAG_OUTER)
    valid2 = np.arange(k2)[None, :] < cnt2[:, None]
    s1 = np.unique(nbr2[valid2])
    nbr1, cnt1 = sampler_ref.sample_neighbors(graph.rowptr, graph.col, s1, k1, key, ops.TAG_INNER)
    kw = {}
    if concat:
        kw["seed_nbr1"], kw["seed_cnt1"] = sampler_ref.sample_neighbors(graph.rowptr, graph.col, seeds, k1, key, ops.TAG_INNER_SELF)
    return ref_sparse.two_hop_forward(table, w1, w2, seeds, nbr2, cnt2, s1, nbr1, cnt1, gcn=not concat, **kw), len(s1), int(cnt1.sum())


@pytest.mark.parametrize("relabel,depth,threads", [("degree", 4, True), ("degree", 4, False), (None, 8, False)])
def test_role_pipeline_at_config3_size_against_the_oracle(relabel, depth, threads):
    """configs[2]: R-MAT 2^20 / 16 M edges, D0 = 256, H = 128/128, fanout 15/25, B = 4096; SGDL, depth 4 with the degree layout
    and one host enqueue thread per role stream (what bench.py times), the same fed by the submitting thread alone, and depth 8 in the caller's order; 2 * depth + 1 batches, so that every workspace is reused at least once.  Every batch's output: (a) bit-identical to the
    single-stream forward of the same (seeds, key); (b) within 1e-5 of the row maximum of the oracle computed from the graph,
    the seeds and the key only."""
    graph = rmat_graph(20, 16_000_000, seed=0, cache_dir=CACHE)
    gen = torch.Generator().manual_seed(0)
    d0, h1, h2, k1, k2, b = 256, 128, 128, 15, 25, 4096
    table = torch.randn(graph.num_nodes, d0, generator=gen)
    w1 = (torch.rand(h1, d0, generator=gen) * 2 - 1) * np.sqrt(6.0 / (h1 + d0))
    w2 = (torch.rand(h2, h1, generator=gen) * 2 - 1) * np.sqrt(6.0 / (h2 + h1))
    cand = np.nonzero(graph.degrees() > 0)[0]
    rs = np.random.default_rng(11)
    nb = 2 * depth + 1
    seeds_host = np.stack([rs.choice(cand, b, replace=False) for _ in range(nb)]).astype(np.int32)
    seeds = torch.from_numpy(seeds_host).to(DEV)
    keys = [0x5A6E355 + i for i in range(nb)]
    rowptr, col = graph.to(DEV)
    tdev, w1d, w2d = table.to(DEV), w1.to(DEV), w2.to(DEV)
    pipe = RolePipeline(rowptr, col, tdev, w1d, w2d, k1, k2, batch=b, depth=depth, roles="SGDL", relabel=relabel, threads=threads)
    assert pipe.threads == threads
    out = torch.empty(nb, b, h2, device=DEV)
    torch.cuda.synchronize()
    for i in range(nb):                                  # one host call per batch, as bench.py's timed loop
        pipe.submit(seeds[i], keys[i], out[i])
    pipe.synchronize()
    torch.cuda.synchronize()
    eng = TwoHopEngine(rowptr, col, tdev, w1d, w2d, k1, k2, max_batch=b, relabel=relabel)
    for i in range(nb):
        assert torch.equal(out[i], eng.forward(seeds[i], seed=keys[i])), f"batch {i}: pipeline differs from the single forward"
    # the oracle works in the ENGINE's node ids (the device sampler is keyed by them): renumber graph, table and seeds on the host
    if relabel == "degree":
        g2, new_of_old = relabel_by_degree(graph)
        assert np.array_equal(eng.node_order.cpu().numpy(), np.argsort(new_of_old, kind="stable"))
        tab2 = table[torch.from_numpy(np.argsort(new_of_old, kind="stable"))]
    else:
        g2, new_of_old, tab2 = graph, None, table
    worst = 0.0
    for i in range(nb):
        sd = seeds_host[i] if new_of_old is None else new_of_old[seeds_host[i]].astype(np.int32)
        ref, n_s1, e1 = oracle_two_hop(g2, tab2, w1, w2, sd, k1, k2, keys[i])
        assert n_s1 > 15_000 and e1 > 200_000           # the full-size frontier, not a degenerate batch
        worst = max(worst, assert_close_rowmax(out[i].cpu(), ref, what=f"pipeline batch {i} vs oracle (relabel={relabel})") or 0.0)
    print(f"role pipeline at config-3 size, relabel={relabel}: {nb} batches, max err / row max = {worst:.2e}")


# ------------------------------------------------------------------------------------------ drop-in training at the engine's speed
from test_gpu_forward import build_modules          # noqa: E402
from util import GOLDEN_DIR, TWO_LAYER_CASES, load_golden, sets_from_padded   # noqa: E402


@pytest.mark.parametrize("cuda", [False, True])
@pytest.mark.parametrize("name", TWO_LAYER_CASES)
def test_module_training_path_through_the_engine_matches_reference_gradients(name, cuda):
    """under grad mode `Encoder.forward` of the two-layer stack (model.py:219-222) is ONE autograd node over
    TwoHopEngine (autograd._TwoHop).  With num_sample >= every set size the device sampler takes whole sets, so on the
    reference's own fixtures (its outputs and ITS autograd's weight gradients on injected sets) the engine path must reproduce
    enc2_out and grad_w1 / grad_w2 -- with the Parameters on the host (cuda=False, the strict drop-in mode) and on the device."""
    g = load_golden(name)
    sets1 = sets_from_padded(g["layer1_nodes"], g["nbr1"], g["cnt1"])
    sets2 = sets_from_padded(g["seeds"], g["nbr2"], g["cnt2"])
    enc1, enc2 = build_modules(g, int(g["k1"]), int(g["k2"]), cuda, sets1, sets2)
    if cuda:
        enc2.to("cuda")                       # nn.Module.to: `.cuda` is shadowed by the flag, as in the reference
    assert enc2._can_fuse_two_hop()
    out = enc2([int(s) for s in g["seeds"]])
    assert out.requires_grad and out.is_cuda == cuda and tuple(out.shape) == g["enc2_out"].shape
    assert enc2._engine is not None and enc2._engine.generation == 1      # the engine ran it, not the per-op path
    assert_close_rowmax(out.detach().cpu(), g["enc2_out"], rows_dim=1, what="forward in grad mode (engine)")
    (out * torch.from_numpy(g["cotangent"]).to(out.device)).sum().backward()
    for got, want, what in ((enc2.weight.grad, g["grad_w2"], "grad_w2"), (enc1.weight.grad, g["grad_w1"], "grad_w1")):
        assert got is not None and got.device == (enc2.weight.device if what == "grad_w2" else enc1.weight.device)
        err = ((got.double().cpu() - torch.from_numpy(want).double()).abs().max() / np.abs(want).max()).item()
        assert err < 5e-5, f"{name} {what}: {err:.2e}"
    # an evaluation forward between loss and backward reuses the workspace: backward then re-runs its forward (same key, same sets)
    enc1.weight.grad = enc2.weight.grad = None
    out = enc2([int(s) for s in g["seeds"]])
    with torch.no_grad():
        enc2([int(s) for s in g["seeds"]][:3])
    (out * torch.from_numpy(g["cotangent"]).to(out.device)).sum().backward()
    err = ((enc1.weight.grad.double().cpu() - torch.from_numpy(g["grad_w1"]).double()).abs().max() / np.abs(g["grad_w1"]).max()).item()
    assert err < 5e-5, f"{name} grad_w1 after an interleaved forward: {err:.2e}"


def _reference_loop(feat_data, labels, adj_lists, num_classes, seed, sample_seed, epochs, batch_size, ref_batching, lr=0.7,
                    hidden1=50, num_sample=10, with_macro=False):
    """graphsage/model.py:192-259 restated with the DROP-IN classes (`from graphsage.encoders import Encoder`, the shim package of
    INTEGRATION.md A) and cuda=False everywhere, as model.py:218-222 effectively runs: seeds, split, SGD lr 0.7, the per-step
    wall clock around loss / backward / step, F1 on the validation split."""
    import random
    import time
    from graphsage.aggregators import MeanAggregator
    from graphsage.encoders import Encoder
    from sklearn.metrics import f1_score
    from sage355.train import SupervisedGraphSage            # model.py:52-69 (the caller's classifier; stock torch)
    np.random.seed(seed)
    random.seed(sample_seed)
    num_nodes = feat_data.shape[0]
    features = torch.nn.Embedding(num_nodes, feat_data.shape[1])
    features.weight = torch.nn.Parameter(torch.FloatTensor(feat_data), requires_grad=False)
    agg1 = MeanAggregator(features, cuda=True)
    enc1 = Encoder(features, feat_data.shape[1], hidden1, adj_lists, agg1, num_sample=num_sample, gcn=True, cuda=False)
    agg2 = MeanAggregator(lambda nodes: enc1(nodes).t(), cuda=False)
    enc2 = Encoder(lambda nodes: enc1(nodes).t(), enc1.embed_dim, 128, adj_lists, agg2, num_sample=num_sample, base_model=enc1, gcn=True, cuda=False)
    graphsage = SupervisedGraphSage(num_classes, enc2)
    rand_indices = np.random.permutation(num_nodes)
    val = rand_indices[int(0.1 * num_nodes):int(0.2 * num_nodes)]
    train = list(rand_indices[int(0.2 * num_nodes):])
    optimizer = torch.optim.SGD(filter(lambda p: p.requires_grad, graphsage.parameters()), lr=lr)
    labels_t = torch.LongTensor(np.asarray(labels))
    times, losses = [], []
    for _ in range(epochs):
        random.shuffle(train)
        for batch in range(0, len(train), batch_size):
            hi = max(len(train), batch + batch_size) if ref_batching else min(len(train), batch + batch_size)
            batch_nodes = train[batch:hi]
            start_time = time.time()
            optimizer.zero_grad()
            loss = graphsage.loss(batch_nodes, labels_t[np.array(batch_nodes)])
            loss.backward()
            optimizer.step()
            times.append(time.time() - start_time)
            losses.append(loss.item())
    val_output = graphsage.forward(val)
    pred = val_output.data.numpy().argmax(axis=1)
    f1 = f1_score(np.asarray(labels)[val].reshape(-1), pred, average="micro")
    if with_macro:                                  # model.py:258 prints it too
        return f1, times, losses, enc2, f1_score(np.asarray(labels)[val].reshape(-1), pred, average="macro")
    return f1, times, losses, enc2


def test_reference_loop_shape_with_the_drop_in_classes_trains_at_engine_speed():
    """The reference's training loop (model.py:240-252), its classes swapped for the drop-in ones by the import line alone,
    cuda=False: <= 1.5 ms per 256-seed step in the median AND <= 2.5 ms in the mean (measured since the cap: median 0.84-0.93 ms, mean
    0.84-0.94 ms over five runs, experiments/r04/call23.sh; round 3: median 0.69, mean 3.15; the reference: 140-180 ms per step on a CPU,
    SURVEY 8c; this path before round 3: 10-12 ms, layer 2 sampled by Python sets).  The F1 of this very loop against the reference's
    distribution over sampling streams is tests/test_gpu_train.py::test_f1_distribution_over_sampling_streams_matches_the_reference
    (path "dropin").
    The mean: the classifier, the loss and SGD of this loop are stock torch ops on the HOST (cuda=False, as model.py
    runs).  On a GPU box torch sees 256 cores behind a 16-core share, and three 70 k-element `add_`s on 256 oversubscribed threads
    took 2 ms each (mean 3-10 ms at a median of 0.7-1.2).  Since round 4 the PRODUCT caps torch's intra-op pool to the usable cores at
    the first cuda=False forward (encoders._cap_host_threads_once), so the test no longer sets the thread count itself."""
    from sage355 import encoders
    from sage355.datasets import standin_citation
    from sage355.graph import CSRGraph
    from util import usable_cores
    z = np.load(os.path.join(GOLDEN_DIR, "cora_topology.npz"))
    g = CSRGraph(z["rowptr"], z["col"], len(z["rowptr"]) - 1)
    feats, labels = standin_citation(g, num_classes=7, feat_dim=1433, seed=0)
    adj = g.to_adj_lists()
    threads = torch.get_num_threads()
    encoders._threads_capped = False               # as in a fresh process: the first cuda=False forward caps the pool
    try:
        torch.manual_seed(0)
        f1, times, losses, enc2 = _reference_loop(feats, labels, adj, 7, 1, 1, 8, 256, False)      # 8 epochs: 72 steps, so that ONE host hiccup of tens
        assert torch.get_num_threads() <= usable_cores()                                             # of milliseconds does not decide the mean
    finally:
        torch.set_num_threads(threads)
    assert enc2._engine is not None and enc2._engine.generation > 0
    steady = times[len(times) // 4:]               # the first epoch warms up (engine construction, CSR conversion, allocator)
    per_step, p80, mean = float(np.median(steady)), float(np.percentile(steady, 80)), float(np.mean(steady))
    print(f"drop-in loop: median {per_step * 1e3:.3f} ms per 256-seed step (80th percentile {p80 * 1e3:.3f}, mean {mean * 1e3:.3f}), F1 {f1:.3f}")
    assert per_step <= 1.5e-3 and p80 <= 3e-3 and mean <= 2.5e-3, (per_step, p80, mean)
    assert f1 > 0.85 and np.mean(losses[-5:]) < 0.6 * np.mean(losses[:5])


# ------------------------------------------------------------------------------------------ reproducible backward
def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


@pytest.mark.parametrize("n,dim,h,concat,act", [(23_000, 256, 128, False, "relu"), (5000, 128, 128, True, "relu"), (300, 100, 52, True, "relu"),
                                                 (129, 50, 7, False, "sigmoid"), (1000, 64, 128, True, "none"), (2816, 1436, 52, False, "relu"),
                                                 (700, 33, 5, True, "relu")])
def test_weight_gradient_through_partials_matches_autograd_and_is_reproducible(n, dim, h, concat, act):
    """sage_linear_act_backward_ws: the fast kernel (even widths: operands straight from HBM in MFMA order) and the generic tile
    kernel (odd widths), both through partial tiles + a fixed-order reduce: against fp64 autograd, and bit-identical across two
    calls (the legacy entry point adds with fp32 atomics, in order of arrival)."""
    from sage355 import autograd, ops
    gen = torch.Generator().manual_seed(n)
    agg = torch.randn(n, dim, generator=gen)
    w = torch.randn(h, dim * (2 if concat else 1), generator=gen) / np.sqrt(dim)
    self_tab = torch.randn(n + 50, dim, generator=gen) if concat else None
    self_index = torch.randperm(n + 50, generator=gen)[:n].to(torch.int32) if concat else None
    cot = torch.randn(n, h, generator=gen)
    code = {"relu": ops.ACT_RELU, "sigmoid": ops.ACT_SIGMOID, "none": ops.ACT_NONE}[act]
    a64, w64 = agg.double().requires_grad_(), w.double().requires_grad_()
    x = torch.cat([self_tab.double()[self_index.long()], a64], 1) if concat else a64
    pre = x.mm(w64.t())
    y = torch.relu(pre) if act == "relu" else torch.sigmoid(pre) if act == "sigmoid" else pre
    (y * cot.double()).sum().backward()
    grads = []
    for _ in range(2):
        ad, wd = agg.to(DEV).requires_grad_(), w.to(DEV).requires_grad_()
        out = autograd.linear_act(ad, wd, code, self_tab.to(DEV) if concat else None, self_index.to(DEV) if concat else None)
        (out * cot.to(DEV)).sum().backward()
        grads.append((wd.grad.clone(), ad.grad.clone()))
    assert _rel(grads[0][0], w64.grad) < 2e-5 and _rel(grads[0][1], a64.grad) < 2e-5
    assert torch.equal(grads[0][0], grads[1][0]) and torch.equal(grads[0][1], grads[1][1])


@pytest.mark.parametrize("dim,self_loop", [(128, False), (52, True), (256, False), (32, True)])
def test_mean_backward_through_the_inverted_index_matches_autograd_and_is_reproducible(dim, self_loop):
    """sage_gather_mean_backward_ws: expand -> stable radix sort by table row -> run heads -> per-row sums in (r, j) order.  Against
    fp64 autograd of the mean (the self row joining the set unless already sampled, as the forward), rows nobody points at come
    out zero, rows past the device-side live count are left alone, and two calls give the same bits."""
    import ctypes
    from sage355 import native
    rs = np.random.default_rng(dim)
    rows, k, n = 3000, 9, 1200
    live = 2500                                           # table rows [live, rows) must not be written
    cnt = rs.integers(0, k + 1, size=n).astype(np.int32)
    nbr = rs.integers(0, live, size=(n, k)).astype(np.int32)
    nbr[:40, :] = 7                                       # a hub: 40 rows x up to 9 slots point at table row 7
    self_row = rs.integers(0, live, size=n).astype(np.int32) if self_loop else None
    g = torch.randn(n, dim, generator=torch.Generator().manual_seed(1))
    # fp64 reference
    want = torch.zeros(rows, dim, dtype=torch.float64)
    for r in range(n):
        ids = list(nbr[r, :cnt[r]])
        if self_loop and int(self_row[r]) not in ids:
            ids.append(int(self_row[r]))
        for t in ids:
            want[t] += g[r].double() / len(ids)
    lib = native.lib()
    need = lib.sage_gather_mean_backward_workspace_bytes(n, k, rows)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    gd, nd, cd = g.to(DEV), torch.from_numpy(nbr).to(DEV), torch.from_numpy(cnt).to(DEV)
    sd = torch.from_numpy(self_row).to(DEV) if self_loop else None
    live_dev = torch.tensor([live], dtype=torch.int32, device=DEV)
    outs = []
    for _ in range(2):
        gt = torch.full((rows, dim), 123.0, device=DEV)
        native.check(lib.sage_gather_mean_backward_ws(native.ptr(gd), gd.stride(0), dim, native.ptr(nd), native.ptr(cd), k, n, None, None,
                                                      native.ptr(sd), native.ptr(gt), rows, native.ptr(live_dev), gt.stride(0), native.ptr(ws),
                                                      ws.numel(), native.stream_handle()), "gather_mean_backward_ws")
        outs.append(gt)
    assert torch.equal(outs[0], outs[1])
    assert bool((outs[0][live:] == 123.0).all()), "rows past the live count were written"
    assert _rel(outs[0][:live], want[:live]) < 2e-6
    untouched = (want[:live].abs().sum(1) == 0)
    assert bool((outs[0][:live][untouched.to(DEV)] == 0).all())


@pytest.mark.parametrize("gcn,relabel,hidden1,d0", [(True, None, 64, 128), (False, "degree", 64, 128), (True, "degree", 30, 66), (True, None, 128, 256)])
def test_training_schedule_is_bitwise_reproducible_eager_and_captured(gcn, relabel, hidden1, d0):
    """Six SGD steps over a ring of four mini-batches: eager twice, captured (ONE hipGraph per step, replayed six times) twice.
    Two eager runs agree BIT FOR BIT in every loss and weight, so do two captured runs, and so do captured and eager (round 2: fp32
    atomics in both backward kernels, and a weight gradient that depended on the frontier's arbitrary row order; round 3: a captured
    hipMemsetAsync that went wrong from its second replay on, and the classifier's gradient left to the BLAS's split of a long
    reduction)."""
    from sage355.train import EngineTrainer
    graph = rmat_graph(14, 300_000, seed=4, accel=None)
    gen = torch.Generator().manual_seed(1)
    table = torch.randn(graph.num_nodes, d0, generator=gen).to(DEV)
    rowptr, col = graph.to(DEV)
    labels_by_node = torch.from_numpy(np.random.default_rng(3).integers(0, 5, graph.num_nodes)).to(DEV)
    cand = np.nonzero(graph.degrees() > 0)[0]
    b = 1024 if d0 == 256 else 256                      # 1024 x 16: layer 1 takes the split (sliced gather + contraction) form
    ring = torch.from_numpy(np.stack([np.random.default_rng(10 + i).choice(cand, b, replace=False) for i in range(4)]).astype(np.int32)).to(DEV)
    keys = [101, 102, 103, 104]

    def make():
        torch.manual_seed(5)
        return EngineTrainer(rowptr, col, table, 5, hidden1=hidden1, hidden2=32, num_sample1=7, num_sample2=15 if d0 == 256 else 9, gcn=gcn,
                             lr=0.3, max_batch=b, relabel=relabel)

    def eager_run():
        tr, losses = make(), []
        for i in range(6):
            j = i % 4
            losses.append(float(tr.step(ring[j], labels_by_node[ring[j].long()], keys[j])))
        return tr, losses

    def captured_run():
        cap = make()
        loss = cap.capture_step(ring, keys, labels_by_node)
        losses = []
        for i in range(6):
            cap.replay_step()
            losses.append(float(loss))
        return cap, losses

    (t1, l1), (t2, l2) = eager_run(), eager_run()
    assert l1 == l2, (l1, l2)
    for name, a, c in zip(("w1", "w2", "w_cls"), t1.parameters(), t2.parameters()):
        assert torch.equal(a, c), f"two eager runs of the same schedule differ in {name}: {(a - c).abs().max().item():.3e} at {int((a != c).sum())} elements"
    (c1, l3), (c2, l4) = captured_run(), captured_run()
    assert l3 == l4, (l3, l4)
    for name, a, c in zip(("w1", "w2", "w_cls"), c1.parameters(), c2.parameters()):
        assert torch.equal(a, c), f"two captured runs of the same schedule differ in {name}: {(a - c).abs().max().item():.3e} at {int((a != c).sum())} elements"
    # captured against eager: bit for bit as well, since the end of round 3 (until then a 16-byte hipMemsetAsync inside the captured step
    # -- the "W holds a huge value" word behind the prepared weight planes -- wrote garbage from its second replay on, ROCm 7.2, and
    # sent layer 1 through the exact fp32 cold path: last-bit differences, experiments/r03/memset_in_graph.py)
    assert l3 == l1, (l3, l1)
    for name, a, c in zip(("w1", "w2", "w_cls"), c1.parameters(), t1.parameters()):
        assert torch.equal(a, c), f"{name}: captured vs eager differ: {(a - c).abs().max().item():.3e} at {int((a != c).sum())} elements"
    assert all(np.isfinite(l1)) and not all(x == l1[0] for x in l1)


# ------------------------------------------------------------------------------------------ the role pipeline as ONE hipGraph
@pytest.mark.parametrize("roles,depth,concat", [("SGDL", 4, False), ("SGDD", 3, True), ("SGDL", 2, False)])
def test_role_pipeline_captured_as_one_graph_replays_bit_identically(roles, depth, concat):
    """fork -> submits -> join over the four role streams captured into one hipGraph (RolePipeline.capture): replayed, every batch
    equals the single-stream forward bit for bit, workspaces are reused inside the graph (3 * depth + 1 batches), a second replay
    gives the same, and eager submission works again afterwards.  The workspace-release edge is an explicit capture dependency
    (csrc/sage_pipe.hip: waiting for it by event crashes hipStreamEndCapture on ROCm 7.2)."""
    graph = rmat_graph(15, 600_000, seed=2, accel=None)
    gen = torch.Generator().manual_seed(0)
    m = 2 if concat else 1
    table = torch.randn(graph.num_nodes, 256, generator=gen).to(DEV)
    w1 = (torch.randn(128, m * 256, generator=gen) / np.sqrt(m * 256)).to(DEV)
    w2 = (torch.randn(64, m * 128, generator=gen) / np.sqrt(m * 128)).to(DEV)
    rowptr, col = graph.to(DEV)
    b, k1, k2 = 1024, 15, 25
    cand = np.nonzero(graph.degrees() > 0)[0]
    rs = np.random.default_rng(5)
    nb = 3 * depth + 1
    seeds = torch.from_numpy(np.stack([rs.choice(cand, b, replace=False) for _ in range(nb)]).astype(np.int32)).to(DEV)
    keys = [1000 + i for i in range(nb)]
    eng = TwoHopEngine(rowptr, col, table, w1, w2, k1, k2, max_batch=b, concat=concat)
    want = [eng.forward(seeds[i], seed=keys[i]).clone() for i in range(nb)]
    pipe = RolePipeline(rowptr, col, table, w1, w2, k1, k2, batch=b, depth=depth, roles=roles, concat=concat)
    out = torch.zeros(nb, b, 64, device=DEV)
    g, st = pipe.capture(seeds, keys, out)
    for rep in range(2):
        out.zero_()
        torch.cuda.synchronize()
        with torch.cuda.stream(st):
            g.replay()
        torch.cuda.synchronize()
        for i in range(nb):
            assert torch.equal(out[i], want[i]), f"replay {rep}, batch {i}: the captured pipeline differs from the single forward"
    out.zero_()
    pipe.submit_many(seeds[:depth + 1], keys[:depth + 1], out)           # eager again after the capture
    pipe.synchronize()
    for i in range(depth + 1):
        assert torch.equal(out[i], want[i])


# ------------------------------------------------------------------------------------------ multi-GPU readiness
import json          # noqa: E402
import subprocess    # noqa: E402
import sys           # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
needs_two_gpus = pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two GPUs (runs on the driver's 8-GPU node; this pool's boxes have one)")


@needs_two_gpus
def test_bench_gpus_2_over_rccl_one_gpu_per_rank():
    """The N > 1 form as the driver runs it: `python bench.py --gpus 2`, backend nccl (= RCCL over xGMI), one GPU per rank, BASELINE
    configs[2] at full size with configs[3] (R-MAT 2^23, the workload BASELINE names for the scaling curve) as a variant."""
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "2", "--steps", "20", "--warmup", "5", "--full", "--cpu-seconds", "0"]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=1500)
    assert res.returncode == 0, res.stderr[-3000:]
    line = json.loads([ln for ln in res.stdout.splitlines() if ln.startswith("{")][-1])
    assert line["n_gpus"] == 2 and line["value"] > 0 and line["scaling"] == "weak" and line["timed_path_check"]["bit_identical_to_oracle_gated_forward"]
    sv = line["config"]["variants"]["configs3_rmat23"]
    assert sv["n_gpus"] == 2 and sv["value"] > 0 and "2^23" in sv["workload"]


def _nccl_dp_rank(rank, world, port, tmp):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                      HSA_ENABLE_IPC_MODE_LEGACY="0")
    from sage355 import dist
    from sage355.train import EngineTrainer
    dist.init_from_env(backend="nccl")
    dev = torch.device("cuda", rank)
    graph = rmat_graph(13, 150_000, seed=4, accel=None)
    table = torch.randn(graph.num_nodes, 66, generator=torch.Generator().manual_seed(1)).to(dev)
    rowptr, col = graph.to(dev)
    torch.manual_seed(10 + rank)
    tr = EngineTrainer(rowptr, col, table, 4, hidden1=30, hidden2=16, num_sample1=5, num_sample2=5, gcn=True, max_batch=128)
    rs = np.random.default_rng(0)
    cand = np.nonzero(graph.degrees() > 0)[0]
    labels_all = torch.from_numpy(rs.integers(0, 4, graph.num_nodes)).to(dev)
    for step in range(6):
        batch = rs.choice(cand, 256, replace=False)
        ids = torch.as_tensor(np.asarray(dist.shard_batch(list(batch), rank, world), dtype=np.int32)).to(dev)
        tr.step(ids, labels_all[ids.long()], key=1000 * rank + step, global_batch=len(batch))
    torch.save(torch.cat([p.reshape(-1).cpu() for p in tr.parameters()]), os.path.join(tmp, f"r{rank}.pt"))
    dist.barrier()
    torch.distributed.destroy_process_group()


@needs_two_gpus
def test_engine_trainer_data_parallel_over_rccl(tmp_path):
    """The nccl twin of test_engine_trainer_data_parallel_one_flat_all_reduce_keeps_replicas_identical: one GPU per rank, ONE flat
    all-reduce of the three weight gradients per step over RCCL; the replicas stay bit-identical."""
    import socket
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    mp.spawn(_nccl_dp_rank, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    assert torch.equal(torch.load(tmp_path / "r0.pt"), torch.load(tmp_path / "r1.pt"))


def test_captured_step_refuses_data_parallel_instead_of_skipping_the_all_reduce(monkeypatch):
    """capture_step records forward + backward + SGD of ONE process; the data-parallel step has a collective between backward and
    SGD, which the captured graph would silently leave out.  It must refuse (world_size > 1), not train replicas apart."""
    from sage355 import dist, native
    from sage355.train import EngineTrainer
    graph = rmat_graph(12, 40_000, seed=4, accel=None)
    table = torch.randn(graph.num_nodes, 64, generator=torch.Generator().manual_seed(1)).to(DEV)
    rowptr, col = graph.to(DEV)
    tr = EngineTrainer(rowptr, col, table, 4, hidden1=32, hidden2=16, num_sample1=5, num_sample2=5, max_batch=64)
    monkeypatch.setattr(dist, "world_size", lambda: 2)
    ring = torch.zeros(2, 64, dtype=torch.int32, device=DEV)
    with pytest.raises(native.SageError, match="single-process"):
        tr.capture_step(ring, [1, 2], torch.zeros(graph.num_nodes, dtype=torch.int64, device=DEV))


# ------------------------------------------------------------------------------------------ self-loop (GCN-variant) aggregator through the backward
@pytest.mark.parametrize("gcn", [True, False])
def test_engine_gradients_with_the_self_loop_aggregator_match_fp64_autograd(gcn):
    """aggregators.py:50-51 (intended semantics; parity-unpinned: the reference line raises TypeError): the node joins its own
    neighbour set unless it was sampled anyway.  The edge-form layer-1 weight gradient carries that as an extra slot per seed;
    checked against fp64 autograd of the set-union means on the sets the engine sampled."""
    from sage355.train import EngineTrainer
    graph = rmat_graph(13, 150_000, seed=4, accel=None)
    d0, h1 = 64, 32
    table = torch.randn(graph.num_nodes, d0, generator=torch.Generator().manual_seed(1)).to(DEV)
    rowptr, col = graph.to(DEV)
    torch.manual_seed(3)
    tr = EngineTrainer(rowptr, col, table, 5, hidden1=h1, hidden2=48, num_sample1=7, num_sample2=9, gcn=gcn, max_batch=300, agg_self_loop=True)
    seeds = np.random.default_rng(2).choice(np.nonzero(graph.degrees() > 0)[0], 300, replace=False)
    labels = torch.from_numpy(np.random.default_rng(3).integers(0, 5, 300)).to(DEV)
    loss, grads = tr.grads(torch.from_numpy(seeds.astype(np.int32)).to(DEV), labels, key=11)
    e = tr.engine
    it = e.intermediates()
    first = it["first_frontier_row"]
    s1 = it["s1_nodes"].cpu().long()
    nbr1, cnt1 = it["nbr1"].cpu().long(), it["cnt1"].cpu().long()
    row2, cnt2 = it["row2"].cpu().long(), it["cnt2"].cpu().long()
    tab = e.table[:, :e.d0].cpu().double()
    w1 = tr.w1.detach().cpu().double().requires_grad_(True)
    w2 = tr.w2.detach().cpu().double().requires_grad_(True)
    wc = tr.w_cls.detach().cpu().double().requires_grad_(True)

    def union_mean(src, idx, cnt, self_idx):
        rows = []
        for r in range(idx.shape[0]):
            members = [int(x) for x in idx[r, :int(cnt[r])]]
            if int(self_idx[r]) not in members:
                members.append(int(self_idx[r]))
            rows.append(src[torch.tensor(members)].mean(0))
        return torch.stack(rows)

    agg1 = union_mean(tab, nbr1, cnt1, s1)                                       # layer 1: the node's own raw row joins
    x1 = torch.cat([tab[s1], agg1], 1) if not gcn else agg1
    hid = torch.relu(x1 @ w1.t())
    pos = {int(v): i for i, v in enumerate(s1.tolist()) if i >= first}            # frontier row of every node id
    self2 = torch.tensor([pos[int(s)] for s in seeds])
    agg2 = union_mean(hid, row2, cnt2, self2)                                    # layer 2: the seed's frontier row joins
    x2 = torch.cat([hid[:len(seeds)], agg2], 1) if not gcn else agg2
    out = torch.relu(x2 @ w2.t())
    ref_loss = torch.nn.functional.cross_entropy(out @ wc.t(), labels.cpu())
    ref = torch.autograd.grad(ref_loss, (w1, w2, wc))
    assert abs(loss.item() - ref_loss.item()) <= 1e-5 * max(1.0, abs(ref_loss.item()))
    for name, g, r in zip(("w1", "w2", "w_cls"), grads, ref):
        err = (g.cpu().double() - r).abs().max().item() / r.abs().max().item()
        assert err <= 2e-5, f"grad {name}: max |g - ref| / max|ref| = {err:.2e}"


# ------------------------------------------------------------------------------------------ host enqueue threads (sage_pipe_set_threads)
@pytest.mark.parametrize("window,concat", [(0, False), (6, False), (3, True)])
def test_role_pipeline_host_threads_are_bit_identical_over_a_long_run(window, concat):
    """One host thread per role stream: 600 batches (more than the descriptor ring holds, so the poster has to wait for the role
    threads; every workspace reused 150 times), with and without a bound on the host's run-ahead, gcn and concat encoders.
    Every output equals the single-stream forward of the same (seeds, key); flush / join / reset / weight updates in between."""
    from sage355 import native
    graph = rmat_graph(14, 200_000, seed=3, cache_dir=CACHE)
    gen = torch.Generator().manual_seed(5)
    d0, h1, h2, k1, k2, b, nb = 64, 32, 16, 5, 7, 256, 600
    mult = 2 if concat else 1
    table = torch.randn(graph.num_nodes, d0, generator=gen).to(DEV)
    w1 = ((torch.rand(h1, mult * d0, generator=gen) * 2 - 1) * 0.2).to(DEV)
    w2 = ((torch.rand(h2, mult * h1, generator=gen) * 2 - 1) * 0.2).to(DEV)
    cand = np.nonzero(graph.degrees() > 0)[0]
    rs = np.random.default_rng(2)
    seeds = torch.from_numpy(np.stack([rs.choice(cand, b, replace=False) for _ in range(nb)]).astype(np.int32)).to(DEV)
    keys = [77 + 13 * i for i in range(nb)]
    rowptr, col = graph.to(DEV)
    pipe = RolePipeline(rowptr, col, table, w1, w2, k1, k2, batch=b, depth=4, roles="SGDL", concat=concat, threads=True, window=window)
    eng = TwoHopEngine(rowptr, col, table, w1, w2, k1, k2, max_batch=b, concat=concat)
    out = torch.empty(nb, b, h2, device=DEV)
    torch.cuda.synchronize()
    for i in range(nb):
        pipe.submit(seeds[i], keys[i], out[i])
    pipe.synchronize()                                   # flushes the role threads, then waits for the four streams
    torch.cuda.synchronize()
    for i in list(range(0, nb, 37)) + [nb - 1]:
        assert torch.equal(out[i], eng.forward(seeds[i], seed=keys[i])), f"batch {i}"
    # submit_many + join on the caller's stream, after a reset; then a weight update seen by the next batch
    pipe.reset()
    out2 = torch.empty(8, b, h2, device=DEV)
    pipe.submit_many(seeds[:8], keys[:8], out2, segment_start=True)
    pipe.join()
    torch.cuda.synchronize()
    assert torch.equal(out2, out[:8])
    with torch.no_grad():
        w2.mul_(0.5)
    pipe.submit(seeds[9], keys[9], out2[0])
    pipe.synchronize()
    torch.cuda.synchronize()
    eng.invalidate_weights()
    assert torch.equal(out2[0], eng.forward(seeds[9], seed=keys[9]))
    assert not torch.equal(out2[0], out[9])
    # threads off again: the submitting thread makes the calls itself, same results
    pipe.set_threads(False)
    pipe.submit(seeds[9], keys[9], out2[1])
    torch.cuda.synchronize()
    assert torch.equal(out2[1], out2[0])
    # a capture in between: the threads step aside (a capture records the calls of the capturing thread) and come back
    pipe.set_threads(True)
    out3 = torch.empty(6, b, h2, device=DEV)
    g, cap_stream = pipe.capture(seeds[20:26], keys[20:26], out3)
    assert pipe.threads
    with torch.cuda.stream(cap_stream):
        g.replay()
    torch.cuda.synchronize()
    for i in range(6):
        assert torch.equal(out3[i], eng.forward(seeds[20 + i], seed=keys[20 + i])), f"captured batch {i}"
    pipe.submit(seeds[30], keys[30], out2[2])            # eager again, through the threads
    pipe.synchronize()
    assert torch.equal(out2[2], eng.forward(seeds[30], seed=keys[30]))
    # the threads need four distinct role streams
    shared = RolePipeline(rowptr, col, table, w1, w2, k1, k2, batch=b, depth=2, roles="SGDD", concat=concat)
    with pytest.raises(native.SageError, match="four distinct role streams"):
        shared.set_threads(True)


# ------------------------------------------------------------------------------------------ the bench line's contract
def test_bench_line_as_the_driver_runs_it_keeps_the_contract():
    """`python bench.py --gpus 1 --steps 20 --warmup 5 --full` (the CPU baseline's budget cut to 3 s here): ONE JSON line on stdout
    with the contract's keys, BASELINE's metric on configs[2], `roofline` and `cpu_baseline` objects whose figures are consistent with
    each other, the timed path's output checked bit for bit, and the 1e-5 parity gate passed."""
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bench.py"), "--gpus", "1",
                        "--steps", "20", "--warmup", "5", "--full", "--cpu-seconds", "3"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, lines
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data",
              "config", "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["metric"].startswith("node-embeddings/sec") and d["unit"] == "embeddings/s" and d["higher_is_better"] is True
    assert (d["n_gpus"], d["steps"], d["warmup"], d["scaling"], d["dtype"], d["data"], d["vs_baseline"]) == (1, 20, 5, "weak", "f32", "synthetic", None)
    cfg = d["config"]
    assert "BASELINE configs[2]" in cfg["workload"] and "model" not in cfg and cfg["batch_per_gpu"] == 4096 and cfg["fanout"] == [15, 25]
    assert abs(d["value"] - 4096 / (d["ms_per_step"] * 1e-3)) <= 1e-3 * d["value"]
    assert d["parity_max_err_vs_fp64_oracle"] <= 1e-5 and d["timed_path_check"]["bit_identical_to_oracle_gated_forward"] is True
    ro = d["roofline"]
    assert ro["bound"] == "hbm" and ro["unit"] == "GB/s" and ro["peak"] == 8000.0
    assert abs(ro["frac"] - ro["achieved"] / ro["peak"]) < 1e-3 and 0.05 < ro["frac"] < 1.0
    assert abs(ro["achieved"] - ro["bytes_per_launch"] / (ro["kernel_ms"] * 1e-3) / 1e9) <= 1e-2 * ro["achieved"]
    assert ro["traffic"] is None or ro["traffic"] >= ro["bytes_per_launch"]           # PMC bytes past L2 cannot be below the algorithmic bytes
    assert abs(ro["forward_frac"] - ro["forward_bytes"] / (d["ms_per_step"] * 1e-3) / 8e12) < 1e-3
    cb = d["cpu_baseline"]
    assert cb["kind"] == "port" and cb["unit"] == "embeddings/s" and cb["cores"] >= 1 and cb["value"] > 0 and "sample" in cb
    assert d["value"] > 1000 * cb["value"]                                 # (a sanity bound, not a target)
    # round 4: BASELINE configs[3] -- the scaling curve's workload -- rides in the N = 1 line, measured by the same code
    v = cfg["variants"]["configs3_rmat23"]
    assert "BASELINE configs[3]" in v["workload"] and "2^23" in v["workload"] and v["n_gpus"] == 1
    assert abs(v["value"] - 4096 / (v["ms_per_step"] * 1e-3)) <= 1e-3 * v["value"]
    assert v["parity_max_err_vs_fp64_oracle"] <= 1e-5 and v["timed_path_check"]["bit_identical_to_oracle_gated_forward"] is True
    assert abs(v["forward_frac"] - v["forward_bytes"] / (v["ms_per_step"] * 1e-3) / 8e12) < 1e-3 and 0.05 < v["forward_frac"] < 1.0
    vr = v["roofline"]
    assert vr["bound"] == "hbm" and abs(vr["achieved"] - vr["bytes_per_launch"] / (vr["kernel_ms"] * 1e-3) / 1e9) <= 1e-2 * vr["achieved"]
    assert v["forward_bytes"] > d["roofline"]["forward_bytes"]           # an 8 x larger graph: fewer duplicates per batch, more unique rows
    # ... and the line says how the pipeline was fed
    h = cfg["host"]
    assert h["ranks_on_node"] == 1 and h["cores_per_rank"] == h["host_cores_usable"] and h["role_threads"] == (h["cores_per_rank"] >= 5)
    assert ("host enqueue thread" in cfg["execution"]) == h["role_threads"]


def test_bench_plain_line_times_only_the_headline_and_dumps_its_last_step(tmp_path):
    """`python bench.py --gpus 1 --steps 20 --warmup 5 --dump-outputs DIR`: ONE JSON line with the contract's keys, `value` consistent
    with `ms_per_step`, nothing that --full adds (no gate, no roofline, no CPU baseline, no variants), and DIR/embeddings.npy = the
    [B, H2] float32 embeddings of the last timed step.  Two runs with the same arguments dump the same bits."""
    dumps = []
    for run in range(2):
        out = tmp_path / f"run{run}"
        r = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bench.py"), "--gpus", "1",
                            "--steps", "20", "--warmup", "5", "--dump-outputs", str(out)], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
        assert len(lines) == 1, lines
        d = json.loads(lines[0])
        assert d["metric"].startswith("node-embeddings/sec") and d["unit"] == "embeddings/s" and d["higher_is_better"] is True
        assert (d["n_gpus"], d["steps"], d["warmup"], d["dtype"]) == (1, 20, 5, "f32")
        assert abs(d["value"] - 4096 / (d["ms_per_step"] * 1e-3)) <= 1e-3 * d["value"]
        assert d["config"]["full"] is False and d["config"]["variants"] is None
        assert d["roofline"] is None and d["cpu_baseline"] is None and d["timed_path_check"] is None
        assert sorted(os.listdir(out)) == ["embeddings.npy"]
        emb = np.load(out / "embeddings.npy")
        assert emb.dtype == np.float32 and emb.shape == (4096, 128) and np.isfinite(emb).all() and (emb != 0).any()
        dumps.append(emb)
    assert np.array_equal(dumps[0], dumps[1])


# ------------------------------------------------------------------------------------------ inference on a pre-transformed table
@pytest.mark.parametrize("relabel,self_loop", [(None, False), ("degree", False), ("degree", True)])
def test_pretransformed_table_inference_matches_the_oracle(relabel, self_loop):
    """engine.pretransform_table: Y = X . W1^T once, then the UNCHANGED engine on (Y, identity, W2).  Same sampled sets as the plain
    engine for the same keys (the sampler never looks at the table), values within the 1e-5 bar of the fp64 oracle of the ORIGINAL
    problem (aggregators.py:54-74, encoders.py:56-61 on X and W1) and within a few fp32 roundings of the plain engine; the role
    pipeline over the transformed table is bit-identical to its single forwards."""
    from sage355.engine import pretransform_table
    import test_gpu_round2 as r2
    graph, table, w1, w2 = r2._problem(scale=15, edges=600_000, d0=256, h1=128, h2=64)
    rowptr, col = graph.to(DEV)
    tdev, w1d, w2d = table.to(DEV), w1.to(DEV), w2.to(DEV)
    b, k1, k2 = 2048, 15, 25
    cand = np.nonzero(graph.degrees() > 0)[0]
    seeds_host = np.random.default_rng(5).choice(cand, b, replace=False).astype(np.int32)
    seeds = torch.from_numpy(seeds_host).to(DEV)
    plain = TwoHopEngine(rowptr, col, tdev, w1d, w2d, k1, k2, max_batch=b, relabel=relabel, agg_self_loop=self_loop)
    y, eye = pretransform_table(tdev, w1d)
    assert y.shape == (graph.num_nodes, 128) and torch.equal(eye, torch.eye(128, device=DEV))
    ref_y = (table.double() @ w1.double().t())
    assert ((y.cpu().double() - ref_y).abs().max() / ref_y.abs().max()).item() < 1e-6          # the library's fp32-accurate contraction
    pre = TwoHopEngine(rowptr, col, y, eye, w2d, k1, k2, max_batch=b, relabel=relabel, agg_self_loop=self_loop)
    assert pre._model().w1_is_identity == 1                    # the marked identity: layer 1 = gather + activation, no contraction launch
    # an UNMARKED identity matrix goes through the contraction (x . 1.0 from the three bf16 terms of x is x): the same bits
    unmarked = TwoHopEngine(rowptr, col, y, torch.eye(128, device=DEV), w2d, k1, k2, max_batch=b, relabel=relabel, agg_self_loop=self_loop)
    assert unmarked._model().w1_is_identity == 0
    assert torch.equal(pre.forward(seeds, seed=77), unmarked.forward(seeds, seed=77))
    with pytest.raises(native_mod.SageError, match="PRE-TRANSFORMED"):
        pre.backward_weights(torch.zeros(b, 64, device=DEV), torch.zeros(b, 64, device=DEV))
    a = plain.forward(seeds, seed=77).clone()
    ia = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in plain.intermediates().items()}
    c = pre.forward(seeds, seed=77).clone()
    ic = pre.intermediates()
    assert ia["n_s1"] == ic["n_s1"] and torch.equal(ia["cnt2"], ic["cnt2"]) and torch.equal(ia["nbr2"], ic["nbr2"])
    # the frontier's row order is arbitrary: compare the layer-1 samples by node
    oa, oc = torch.argsort(ia["s1_nodes"]), torch.argsort(ic["s1_nodes"])
    assert torch.equal(ia["s1_nodes"][oa], ic["s1_nodes"][oc]) and torch.equal(ia["nbr1"][oa], ic["nbr1"][oc])
    scale = a.abs().amax(1, keepdim=True).clamp_min(1e-30)
    assert ((a - c).abs() / scale).max().item() < 5e-6
    # the fp64 oracle of the original problem on the sets the GPU drew (ids are the engine's internal ones)
    it = {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in ic.items()}
    first = it["first_frontier_row"]
    seeds_int = seeds_host if pre._new_of_old is None else pre._new_of_old[seeds.long()].cpu().numpy()
    ref = ref_sparse.two_hop_forward(plain.table.cpu(), w1, w2, seeds_int, it["nbr2"], it["cnt2"], it["s1_nodes"][first:], it["nbr1"][first:],
                                     it["cnt1"][first:], gcn=True, agg_gcn=self_loop)
    assert_close_rowmax(c.cpu(), ref, what="pre-transformed engine vs oracle")
    # the throughput path over the transformed table
    pipe = RolePipeline(rowptr, col, y, eye, w2d, k1, k2, batch=b, depth=3, relabel=relabel, agg_self_loop=self_loop, threads=True)
    out = torch.empty(5, b, 64, device=DEV)
    sd = torch.stack([seeds, seeds.flip(0), seeds.roll(3), seeds, seeds.roll(9)])
    for i in range(5):
        pipe.submit(sd[i], 100 + i, out[i])
    pipe.synchronize()
    for i in range(5):
        assert torch.equal(out[i], pre.forward(sd[i], seed=100 + i))
    with pytest.raises(native_mod.SageError):
        pretransform_table(tdev, torch.zeros(128, 512, device=DEV))          # the concat encoder's [H1, 2 D0] weight: not supported
