"""GPU tests of the two-layer stack at fanouts above 64 (twohop_ops.two_hop_forward and the Encoder routes to it; run with -m gpu).

Integer sets are compared bit for bit with test_sample_wide_host.wide_ref (the Python restatement of oracle/sampler_ref.c's rule), the
output with the fp64 oracle on the very same sets under util.assert_close_rowmax (RTOL = 1e-5 of the row maximum, the gate of every
forward test), the weight gradients with torch autograd in fp64 under the 5e-5 of tests/test_gpu_backward.py."""
import random

import numpy as np
import pytest
import torch

from oracle import ref_sparse
from sage355 import native, ops
from sage355.aggregators import MeanAggregator
from sage355.encoders import Encoder
from sage355.engine import TwoHopEngine
from sage355.graph import rmat_graph
from sage355.twohop_ops import two_hop_forward
from test_sample_wide_host import wide_ref
from util import assert_close_rowmax, torch_two_hop

pytestmark = pytest.mark.gpu
DEV = "cuda"
D0, H1, H2 = 64, 32, 16
KEY = 0x5EED0123456789AB
VARIANTS = [(False, False), (True, False), (False, True), (True, True)]      # (concat, agg_self_loop)


@pytest.fixture(scope="module")
def setup():
    g = rmat_graph(13, 200_000, seed=3)
    gen = torch.Generator().manual_seed(0)
    table = torch.randn(g.num_nodes, D0, generator=gen)
    weights = {concat: (torch.randn(H1, D0 * m, generator=gen) / np.sqrt(D0 * m), torch.randn(H2, H1 * m, generator=gen) / np.sqrt(H1 * m))
               for concat, m in ((False, 1), (True, 2))}
    return g, torch.from_numpy(g.rowptr).to(DEV), torch.from_numpy(g.col).to(DEV), table, weights


def positive_degree_seeds(g, b, seed=0):
    return np.random.default_rng(seed).choice(np.nonzero(g.degrees() > 0)[0], b, replace=False).astype(np.int32)


def host_sets(sets):
    return {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in sets.items()}


def oracle_on_sets(table, w1, w2, seeds, s, concat, self_loop):
    first = s["first_frontier_row"]
    return ref_sparse.two_hop_forward(table, w1, w2, seeds, s["nbr2"], s["cnt2"], s["s1_nodes"][first:], s["nbr1"][first:], s["cnt1"][first:],
                                      gcn=not concat, agg_gcn=self_loop, seed_nbr1=s["nbr1"][:first] if concat else None,
                                      seed_cnt1=s["cnt1"][:first] if concat else None)


@pytest.mark.parametrize("concat,self_loop", VARIANTS)
def test_two_hop_forward_wide_against_the_oracle(setup, concat, self_loop):
    g, rowptr, col, table, weights = setup
    w1, w2 = weights[concat]
    k1, k2, b = 80, 100, 300
    seeds = positive_degree_seeds(g, b)
    out, sets = two_hop_forward(rowptr, col, table.to(DEV), w1.to(DEV), w2.to(DEV), torch.from_numpy(seeds).to(DEV), k1, k2, KEY,
                                concat=concat, agg_self_loop=self_loop, return_sets=True)
    assert out.shape == (b, H2)
    s = host_sets(sets)
    first, s1 = s["first_frontier_row"], s["s1_nodes"]
    assert first == (b if concat else 0) and s["n_s1"] == len(s1) == len(s["nbr1"]) == len(s["cnt1"])
    # the outer sets, all of them; the inner sets, a random 500 rows (seed rows of the concat encoder draw from their own stream)
    r2, c2 = wide_ref(g.rowptr, g.col, seeds, k2, KEY, ops.TAG_OUTER)
    assert np.array_equal(s["nbr2"], r2) and np.array_equal(s["cnt2"], c2)
    if concat:
        assert np.array_equal(s1[:first], seeds)
    rows = np.random.default_rng(1).choice(len(s1), 500, replace=False)
    for part, tag in ((rows[rows < first], ops.TAG_INNER_SELF), (rows[rows >= first], ops.TAG_INNER)):
        r1, c1 = wide_ref(g.rowptr, g.col, s1[part], k1, KEY, tag)
        assert np.array_equal(s["nbr1"][part], r1) and np.array_equal(s["cnt1"][part], c1)
    assert (s["cnt1"] == np.minimum(g.degrees()[s1], k1)).all() and (g.degrees()[s1] > k1).sum() > 100       # both branches of the draw
    # the frontier is the union of the outer sets (with the seeds under the gcn aggregator)
    valid2 = np.arange(k2)[None, :] < c2[:, None]
    expect = set(r2[valid2].tolist()) | (set(seeds.tolist()) if self_loop else set())
    assert set(s1[first:].tolist()) == expect and len(s1) - first == len(expect)
    ref = oracle_on_sets(table, w1, w2, seeds, s, concat, self_loop)
    assert_close_rowmax(out.cpu(), ref, what=f"two_hop_forward concat={concat} self_loop={self_loop}")


def test_isolated_seed_follows_the_reference_nan_rule(setup):
    g, rowptr, col, table, weights = setup
    w1, w2 = weights[False]
    isolated = np.nonzero(g.degrees() == 0)[0]
    assert isolated.size > 0
    seeds = positive_degree_seeds(g, 40)
    seeds[7] = isolated[0]
    out, sets = two_hop_forward(rowptr, col, table.to(DEV), w1.to(DEV), w2.to(DEV), torch.from_numpy(seeds).to(DEV), 80, 100, KEY,
                                return_sets=True)
    s = host_sets(sets)
    assert s["cnt2"][7] == 0
    ref = oracle_on_sets(table, w1, w2, seeds, s, False, False)
    assert torch.isnan(ref[7]).all() and not torch.isnan(ref[:7]).any()       # the reference's 0/0 inside a mixed batch
    assert_close_rowmax(out.cpu(), ref, what="isolated seed")                  # NaN patterns must coincide


@pytest.mark.parametrize("concat,self_loop", VARIANTS)
def test_narrow_fanouts_give_the_engine_sets(setup, concat, self_loop):
    g, rowptr, col, table, weights = setup
    w1, w2 = weights[concat]
    k1, k2, b = 10, 20, 200
    seeds = torch.from_numpy(positive_degree_seeds(g, b, seed=2)).to(DEV)
    eng = TwoHopEngine(rowptr, col, table.to(DEV), w1.to(DEV), w2.to(DEV), k1, k2, concat=concat, agg_self_loop=self_loop, max_batch=b)
    out_e = eng.forward(seeds, seed=KEY).cpu()
    e = host_sets(eng.intermediates())
    out, sets = two_hop_forward(rowptr, col, table.to(DEV), w1.to(DEV), w2.to(DEV), seeds, k1, k2, KEY, concat=concat,
                                agg_self_loop=self_loop, return_sets=True)
    s = host_sets(sets)
    first = s["first_frontier_row"]
    assert first == e["first_frontier_row"] and s["n_s1"] == e["n_s1"]
    assert np.array_equal(s["nbr2"], e["nbr2"]) and np.array_equal(s["cnt2"], e["cnt2"])
    assert np.array_equal(s["s1_nodes"][:first], e["s1_nodes"][:first])
    assert np.array_equal(s["nbr1"][:first], e["nbr1"][:first]) and np.array_equal(s["cnt1"][:first], e["cnt1"][:first])
    # the order of the frontier rows is arbitrary on both sides: compare them by node id
    so, eo = first + np.argsort(s["s1_nodes"][first:]), first + np.argsort(e["s1_nodes"][first:])
    assert np.array_equal(s["s1_nodes"][so], e["s1_nodes"][eo])
    assert np.array_equal(s["nbr1"][so], e["nbr1"][eo]) and np.array_equal(s["cnt1"][so], e["cnt1"][eo])
    assert_close_rowmax(out.cpu(), out_e.double(), what=f"operators vs engine concat={concat} self_loop={self_loop}")


@pytest.mark.parametrize("concat", [False, True])
def test_weight_gradients_match_fp64_autograd(setup, concat):
    g, rowptr, col, table, weights = setup
    w1, w2 = weights[concat]
    k1, k2, b = 70, 90, 64
    seeds = positive_degree_seeds(g, b, seed=3)
    w1d, w2d = w1.to(DEV).requires_grad_(), w2.to(DEV).requires_grad_()
    out, sets = two_hop_forward(rowptr, col, table.to(DEV), w1d, w2d, torch.from_numpy(seeds).to(DEV), k1, k2, KEY, concat=concat,
                                return_sets=True)
    cot = torch.randn(b, H2, generator=torch.Generator().manual_seed(5))
    (out * cot.to(DEV)).sum().backward()
    s = host_sets(sets)
    # util.torch_two_hop finds a node's layer-1 row by id.  The concat encoder evaluates layer 1 on a seed twice (as seed, on its own
    # samples, and as a frontier node when it was sampled): the seed rows get ids of their own past the table, with the seeds' features.
    t64 = table.double()
    n = g.num_nodes
    if concat:
        t64 = torch.cat([t64, t64[torch.from_numpy(seeds).long()]])
        layer1_nodes = np.concatenate([n + np.arange(b), s["s1_nodes"][b:]])
        fix_seeds = n + np.arange(b)
    else:
        layer1_nodes, fix_seeds = s["s1_nodes"], seeds
    fixture = {"gcn": not concat, "layer1_nodes": layer1_nodes.astype(np.int64), "nbr1": s["nbr1"], "cnt1": s["cnt1"], "nbr2": s["nbr2"],
               "cnt2": s["cnt2"], "seeds": fix_seeds}
    w1r, w2r = w1.double().requires_grad_(), w2.double().requires_grad_()
    ref = torch_two_hop(t64, w1r, w2r, fixture)
    assert_close_rowmax(out.detach().cpu(), ref.detach(), what="forward in grad mode")
    (ref * cot.double()).sum().backward()
    for got, want, what in ((w2d.grad, w2r.grad, "grad_w2"), (w1d.grad, w1r.grad, "grad_w1")):
        err = ((got.double().cpu() - want).abs().max() / want.abs().max().clamp_min(1e-30)).item()
        print(f"concat={concat} {what}: rel_err = {err:.2e}")
        assert err < 5e-5, f"{what}: {err:.2e}"


def build_stack(g, table, num_sample, gcn):
    """model.py:214-222 with this package's classes."""
    adj = {v: set(g.neighbors(v).tolist()) for v in range(g.num_nodes)}
    features = torch.nn.Embedding(*table.shape)
    features.weight = torch.nn.Parameter(table.clone(), requires_grad=False)
    agg1 = MeanAggregator(features, cuda=False)
    enc1 = Encoder(features, table.shape[1], H1, adj, agg1, num_sample=num_sample, gcn=gcn, cuda=False)
    agg2 = MeanAggregator(lambda nodes: enc1(nodes).t(), cuda=False)
    enc2 = Encoder(lambda nodes: enc1(nodes).t(), enc1.embed_dim, H2, adj, agg2, num_sample=num_sample, base_model=enc1, gcn=gcn, cuda=False)
    return enc1, enc2


def no_host_sampling(monkeypatch):
    def refuse(*args, **kwargs):
        raise AssertionError("random.sample was called: the forward left the device path")
    monkeypatch.setattr(random, "sample", refuse)


@pytest.mark.parametrize("gcn", [True, False])
def test_drop_in_stack_with_num_sample_100_stays_on_the_device(setup, monkeypatch, gcn):
    g, _, _, table, _ = setup
    enc1, enc2 = build_stack(g, table, 100, gcn)
    assert enc2._can_two_hop_ops() and not enc2._can_fuse_two_hop()
    no_host_sampling(monkeypatch)
    seeds = [int(x) for x in positive_degree_seeds(g, 96, seed=4)]
    random.seed(1)
    with torch.no_grad():
        out = enc2(seeds)
    assert tuple(out.shape) == (H2, len(seeds)) and not out.is_cuda and not out.requires_grad
    assert torch.isfinite(out).all() and out.abs().sum() > 0
    random.seed(1)
    out_g = enc2(seeds)
    assert out_g.requires_grad and torch.equal(out_g.detach(), out)        # random.seed() still makes a run reproducible
    out_g.sum().backward()
    for enc in (enc1, enc2):
        assert enc.weight.grad is not None and torch.isfinite(enc.weight.grad).all() and enc.weight.grad.abs().sum() > 0


def test_single_table_encoder_with_num_sample_100_takes_the_table_path(setup, monkeypatch):
    g, _, _, table, _ = setup
    enc1, _ = build_stack(g, table, 100, True)
    no_host_sampling(monkeypatch)
    taken = []
    table_path = enc1._forward_table
    monkeypatch.setattr(enc1, "_forward_table", lambda nodes: taken.append("table") or table_path(nodes))
    monkeypatch.setattr(enc1, "_forward_generic", lambda nodes: taken.append("generic"))
    seeds = [int(x) for x in positive_degree_seeds(g, 96, seed=4)]
    with torch.no_grad():
        out = enc1(seeds)
    assert taken == ["table"] and tuple(out.shape) == (H1, len(seeds)) and torch.isfinite(out).all()
    enc1.num_sample = native.MAX_FANOUT_WIDE + 1                           # beyond the wide sampler: the strict path, as before
    taken.clear()
    monkeypatch.setattr(enc1, "_forward_generic", lambda nodes: taken.append("generic") or torch.zeros(len(nodes), H1, device=DEV))
    enc1(seeds)
    assert taken == ["generic"]
