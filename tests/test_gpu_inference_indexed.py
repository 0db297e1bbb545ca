"""Whole-graph inference through a trainable embedding (the 1hot / node_degree initializers, aggregators.py:30-31, 68-71):
embed_all_nodes(table=embed, index=ix) against embed_all_nodes(table=embed[ix]) bit for bit, and embed_all_from_modules on the
reference's own initializer stacks (tests/golden/tiny_1hot.npz, tiny_node_degree.npz) with what it refuses."""
import numpy as np
import pytest
import torch

from sage355 import native, ops
from sage355.graph import rmat_graph
from sage355.inference import embed_all_from_modules, embed_all_nodes, layer_all_nodes
from test_gpu_initializer_modules import CASES, build
from util import RTOL, assert_close_rowmax, full_table, load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda"


def bits_equal(a, b):
    """Bitwise equality, NaNs included (torch.equal says NaN != NaN)."""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def one_hot_table(g):
    """The fixture stores the feature rows the reference touched and full_table leaves the others zero; the whole-graph run reads
    every row, so the others become one-hots too (column 0: they are no node's neighbour and no seed, so no checked row sees them)."""
    table = full_table(g)
    table[~(table == 1).any(1), 0] = 1.0
    return table


@pytest.fixture(scope="module")
def rmat():
    g = rmat_graph(13, 60_000, seed=4, accel=None)
    deg = g.degrees()
    assert g.num_nodes == 8192 and int(deg.max()) > 2 * native.CSR_MEAN_CHUNK and (deg == 0).any()
    rp, cl = g.to(DEV)
    return g, rp, cl, torch.from_numpy(deg.astype(np.int32)).to(DEV), int(deg.max()) + 1


@pytest.mark.parametrize("rows_per_call", [1 << 18, 3000])
@pytest.mark.parametrize("sigmoid", [False, True], ids=["relu", "sigmoid"])
@pytest.mark.parametrize("gcn,self_loop", [(True, False), (True, True), (False, False), (False, True)])
def test_embed_all_nodes_through_an_index_is_the_materialised_run_bit_for_bit(rmat, gcn, self_loop, sigmoid, rows_per_call):
    g, rp, cl, ix, k = rmat
    d0, h1, h2 = 64, 50, 16
    gen = torch.Generator(device=DEV).manual_seed(7)
    mult = 1 if gcn else 2
    embed = torch.randn(k, d0, device=DEV, generator=gen)
    w1 = torch.randn(h1, mult * d0, device=DEV, generator=gen) / 8
    w2 = torch.randn(h2, mult * h1, device=DEV, generator=gen) / 7
    kw = dict(concat=not gcn, agg_self_loop=self_loop, act1=ops.ACT_SIGMOID if sigmoid else ops.ACT_RELU, rows_per_call=rows_per_call)
    want = embed_all_nodes(rp, cl, embed[ix.long()], w1, w2, **kw)
    got = embed_all_nodes(rp, cl, embed, w1, w2, index=ix, **kw)
    assert tuple(got.shape) == (g.num_nodes, h2) and bits_equal(got, want)
    assert bool(torch.isnan(got).any()) != self_loop, "isolated nodes: NaN rows unless the node itself joins its mean"
    one = layer_all_nodes(rp, cl, embed, w1, not gcn, self_loop, kw["act1"], rows_per_call=rows_per_call, index=ix)
    assert bits_equal(one, layer_all_nodes(rp, cl, embed[ix.long()], w1, not gcn, self_loop, kw["act1"], rows_per_call=rows_per_call))


def test_embed_all_nodes_checks_the_index_once(rmat):
    g, rp, cl, ix, k = rmat
    embed = torch.randn(k, 8, device=DEV)
    w1, w2 = torch.randn(4, 8, device=DEV), torch.randn(4, 4, device=DEV)
    with pytest.raises(native.SageError):
        embed_all_nodes(rp, cl, embed[:-1], w1, w2, index=ix)                       # the largest degree has no row
    bad = ix.clone()
    bad[5] = -1
    with pytest.raises(native.SageError):
        embed_all_nodes(rp, cl, embed, w1, w2, index=bad)
    with pytest.raises(native.SageError):
        embed_all_nodes(rp, cl, embed, w1, w2, index=ix[:-1].contiguous())
    with pytest.raises(native.SageError):
        embed_all_nodes(rp, cl, embed, w1, w2, index=ix.long())


@pytest.mark.parametrize("cuda", [False, True])
@pytest.mark.parametrize("name", sorted(CASES))
def test_embed_all_from_modules_on_the_initializer_stacks(name, cuda):
    g = load_golden(name)
    agg1, enc1, enc2, _ = build(g, CASES[name], cuda, None, None, table=one_hot_table(g))
    emb = embed_all_from_modules(enc2, rows_per_call=7)
    n = enc1.features.weight.shape[0]
    assert emb.is_cuda and tuple(emb.shape) == (n, enc2.weight.shape[0])
    seeds = [int(s) for s in g["seeds"]]
    with torch.no_grad():
        ref = enc2(seeds)                                      # num_sample=None: the strict path, [h2, B]
    assert_close_rowmax(emb.cpu()[torch.tensor(seeds)].t(), g["enc2_out"], rtol=RTOL, rows_dim=1, what=f"{name} vs reference")
    assert_close_rowmax(emb.cpu()[torch.tensor(seeds)].t(), ref.detach().cpu(), rtol=RTOL, rows_dim=1, what=f"{name} vs enc2(seeds)")


@pytest.mark.parametrize("name", sorted(CASES))
def test_embed_all_from_modules_refusals(name):
    g = load_golden(name)
    init = CASES[name]
    table = one_hot_table(g)
    victim = int(g["nbr1"][0, 0])
    table[victim] = 0.0
    table[victim, 0] = 0.5
    _, _, enc2, _ = build(g, init, False, None, None, table=table)
    with pytest.raises(native.SageError, match="no element equal to 1"):
        embed_all_from_modules(enc2)
    agg1, enc1, enc2, _ = build(g, init, False, None, None, table=one_hot_table(g))
    assert embed_all_from_modules(enc2).shape[0] == enc1.features.weight.shape[0]
    enc2.initializer = init                                    # an initializer on the outer encoder
    with pytest.raises(native.SageError, match="outer"):
        embed_all_from_modules(enc2)
    enc2.initializer = "None"
    enc1.gcn = enc2.gcn = False                                # the concat encoder: the reference feeds the raw one-hot there
    with pytest.raises(native.SageError, match="concat"):
        embed_all_from_modules(enc2)
    enc1.gcn = enc2.gcn = True
    full = agg1.embed
    agg1.embed = torch.nn.Embedding(1, full.weight.shape[1])  # an index past the embedding's rows
    with pytest.raises(native.SageError, match="outside the embedding"):
        embed_all_from_modules(enc2)
    del agg1.embed                                             # an aggregator without `embed`
    with pytest.raises(native.SageError, match="embed"):
        embed_all_from_modules(enc2)
    agg1.embed = full
    assert embed_all_from_modules(enc2).shape[0] == enc1.features.weight.shape[0]
