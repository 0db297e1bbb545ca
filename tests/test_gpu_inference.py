"""Whole-graph layer-wise inference (sage355.inference) on the MI355X: the reference's own num_sample=None outputs, the fp64
oracle on a skewed R-MAT graph, and the module entry point."""
import numpy as np
import pytest
import torch

from oracle import ref_dense
from sage355 import native, ops
from sage355.graph import csr_from_adj_lists, rmat_graph
from sage355.inference import embed_all_from_modules, embed_all_nodes
from test_gpu_forward import build_modules
from util import TWO_LAYER_CASES, assert_close_rowmax, full_table, load_golden, sets_from_padded

pytestmark = pytest.mark.gpu


def bits_equal(a, b):
    """Bitwise equality, NaNs included (torch.equal says NaN != NaN)."""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def act_of(flag):
    return ops.ACT_SIGMOID if int(flag) else ops.ACT_RELU


@pytest.mark.parametrize("name", TWO_LAYER_CASES)
def test_embed_all_nodes_reproduces_reference_goldens(name):
    """Inner CSR = the fixture's layer-1 sets, outer CSR = its seeds' sets: rows [seeds] are the reference's enc2 output."""
    g = load_golden(name)
    table = full_table(g)
    n = table.shape[0]
    rp1, c1 = csr_from_adj_lists(sets_from_padded(g["layer1_nodes"], g["nbr1"], g["cnt1"]), num_nodes=n).to("cuda")
    rp2, c2 = csr_from_adj_lists(sets_from_padded(g["seeds"], g["nbr2"], g["cnt2"]), num_nodes=n).to("cuda")
    out = embed_all_nodes(rp1, c1, table.cuda(), torch.from_numpy(g["w1"]).cuda(), torch.from_numpy(g["w2"]).cuda(),
                          concat=not bool(g["gcn"]), act1=act_of(g["sigmoid1"]), act2=act_of(g["sigmoid2"]),
                          rowptr_outer=rp2, col_outer=c2, rows_per_call=997)      # several row blocks
    seeds = torch.from_numpy(g["seeds"].astype(np.int64))
    assert_close_rowmax(out.cpu()[seeds].t(), g["enc2_out"], rows_dim=1, what=f"{name} enc2_out")


@pytest.fixture(scope="module")
def rmat13():
    g = rmat_graph(13, 150_000, seed=4)
    deg = g.degrees()
    rng = np.random.default_rng(4)
    isolated = np.nonzero(deg == 0)[0]
    assert isolated.size >= 2 and int(deg.max()) > 4 * native.CSR_MEAN_CHUNK
    others = rng.choice(np.nonzero(deg > 0)[0], 250, replace=False)
    seeds = np.unique(np.concatenate([[int(np.argmax(deg))], isolated[:3], others]))
    return g, g.to_adj_lists(), seeds


@pytest.mark.parametrize("gcn,sigmoid,self_loop", [(True, False, False), (True, True, True), (False, False, True), (False, True, False)])
def test_embed_all_nodes_against_fp64_oracle(rmat13, gcn, sigmoid, self_loop):
    g, adj, seeds = rmat13
    d0, h1, h2 = 64, 50, 16
    gen = torch.Generator().manual_seed(7)
    mult = 1 if gcn else 2
    table = torch.randn(g.num_nodes, d0, generator=gen)
    w1 = torch.randn(h1, mult * d0, generator=gen) / 8
    w2 = torch.randn(h2, mult * h1, generator=gen) / 7
    rp, cl = g.to("cuda")
    act = ops.ACT_SIGMOID if sigmoid else ops.ACT_RELU
    out = embed_all_nodes(rp, cl, table.cuda(), w1.cuda(), w2.cuda(), concat=not gcn, agg_self_loop=self_loop, act1=act, act2=act,
                          rows_per_call=3000)
    init = "shared" if sigmoid else "None"
    prev = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)          # the oracle's dense masks in fp64 too
    try:
        ref = ref_dense.two_hop_forward([int(s) for s in seeds], adj, adj, table.double(), w1.double(), w2.double(), None, None, gcn,
                                        self_loop, initializer1=init, initializer2=init)
    finally:
        torch.set_default_dtype(prev)
    assert_close_rowmax(out.cpu()[torch.from_numpy(seeds)].t(), ref, rows_dim=1, what=f"gcn={gcn} sigmoid={sigmoid} self_loop={self_loop}")


@pytest.mark.parametrize("name", ["tiny_sigmoid", "cora_emb_gcn_5_5", "cora_emb_concat_10_10", "pubmed_concat_10_25"])
def test_embed_all_from_modules(name):
    g = load_golden(name)
    sets1 = sets_from_padded(g["layer1_nodes"], g["nbr1"], g["cnt1"])
    sets2 = sets_from_padded(g["seeds"], g["nbr2"], g["cnt2"])
    enc1, enc2 = build_modules(g, None, None, False, sets1, sets2)
    emb = embed_all_from_modules(enc2)
    n = enc1.features.weight.shape[0]
    rp1, c1 = csr_from_adj_lists(sets1, num_nodes=n).to("cuda")
    rp2, c2 = csr_from_adj_lists(sets2, num_nodes=n).to("cuda")
    direct = embed_all_nodes(rp1, c1, enc1.features.weight.detach().cuda(), enc1.weight.detach().cuda(), enc2.weight.detach().cuda(),
                             concat=not enc1.gcn, act1=enc1._act(), act2=enc2._act(), rowptr_outer=rp2, col_outer=c2)
    assert bits_equal(emb, direct)
    seeds = [int(s) for s in g["seeds"]]
    with torch.no_grad():
        ref = enc2(seeds)                                      # num_sample=None: the strict path, [h2, B]
    assert_close_rowmax(emb.cpu()[torch.tensor(seeds)].t(), ref, rows_dim=1, what=f"{name} vs enc2(seeds)")
    assert_close_rowmax(emb.cpu()[torch.tensor(seeds)].t(), g["enc2_out"], rows_dim=1, what=f"{name} vs reference")


def test_embed_all_from_modules_refuses_other_setups():
    g = load_golden("tiny_gcn")
    sets1 = sets_from_padded(g["layer1_nodes"], g["nbr1"], g["cnt1"])
    sets2 = sets_from_padded(g["seeds"], g["nbr2"], g["cnt2"])
    enc1, enc2 = build_modules(g, None, None, False, sets1, sets2)
    with pytest.raises(native.SageError):
        embed_all_from_modules(enc1)                           # no base model
    enc1.initializer = "node_degree"
    with pytest.raises(native.SageError):
        embed_all_from_modules(enc2)
    enc1.initializer = "None"
    feats = enc1.features
    del enc1.features                                          # a submodule: unregister it before putting a function there
    enc1.features = lambda ids: feats(ids)                     # not a feature table
    with pytest.raises(native.SageError):
        embed_all_from_modules(enc2)
    del enc1.features
    enc1.features = feats
    agg = enc2.aggregator
    enc2.aggregator = torch.nn.Identity()                      # a foreign aggregator
    with pytest.raises(native.SageError):
        embed_all_from_modules(enc2)
    enc2.aggregator = agg
    assert embed_all_from_modules(enc2).shape == (enc1.features.weight.shape[0], enc2.weight.shape[0])
