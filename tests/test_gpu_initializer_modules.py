"""The drop-in modules with the reference's 1hot / node_degree initializers (aggregators.py:30-31, 68-71): the feature rows are
one-hots that index a trainable nn.Embedding kept by the layer-1 aggregator.  Outputs and gradients against the reference's own
(tests/golden/tiny_1hot.npz, tiny_node_degree.npz, written by tests/golden/make_golden_initializers.py), and the routing of
Encoder.forward."""
import numpy as np
import pytest
import torch

from sage355 import native
from sage355.aggregators import MeanAggregator
from sage355.encoders import Encoder
from util import RTOL, assert_close_rowmax, full_table, load_golden, sets_from_padded

pytestmark = pytest.mark.gpu
CASES = {"tiny_1hot": "1hot", "tiny_node_degree": "node_degree"}


def build(g, initializer, cuda, num_sample1, num_sample2, table=None):
    """model.py:214-222 wiring with this package's classes; the initializer goes to the layer-1 aggregator and encoder only."""
    table = full_table(g) if table is None else table
    sets1 = sets_from_padded(g["layer1_nodes"], g["nbr1"], g["cnt1"])
    sets2 = sets_from_padded(g["seeds"], g["nbr2"], g["cnt2"])
    rows, width = g["embed"].shape
    assert width == int(g["embed_dim"]) and width != table.shape[1], "the embedding must not be as wide as the one-hot"
    features = torch.nn.Embedding(*table.shape)
    features.weight = torch.nn.Parameter(table, requires_grad=False)
    agg1 = MeanAggregator(features, cuda=cuda, feature_dim=width, num_nodes=rows, initializer=initializer)
    enc1 = Encoder(features, width, g["w1"].shape[0], sets1, agg1, num_sample=num_sample1, gcn=True, cuda=cuda, initializer=initializer)
    agg2 = MeanAggregator(lambda nodes: enc1(nodes).t(), cuda=cuda)
    enc2 = Encoder(lambda nodes: enc1(nodes).t(), enc1.embed_dim, g["w2"].shape[0], sets2, agg2, num_sample=num_sample2, base_model=enc1,
                   gcn=True, cuda=cuda)
    with torch.no_grad():
        enc1.weight.copy_(torch.from_numpy(g["w1"]))
        enc2.weight.copy_(torch.from_numpy(g["w2"]))
        agg1.embed.weight.copy_(torch.from_numpy(g["embed"]))
    if cuda:
        enc2.to("cuda")                       # nn.Module.to: `.cuda` is shadowed by the flag, as in the reference
    return agg1, enc1, enc2, sets1


def _check_against_the_golden(g, agg1, enc1, enc2, cuda, what):
    out = enc2([int(s) for s in g["seeds"]])
    assert out.requires_grad and out.is_cuda == cuda and tuple(out.shape) == g["enc2_out"].shape
    assert_close_rowmax(out.detach().cpu(), g["enc2_out"], rtol=RTOL, rows_dim=1, what=f"{what} enc2(seeds)")
    (out * torch.from_numpy(g["cotangent"]).to(out.device)).sum().backward()
    for got, key in ((agg1.embed.weight.grad, "grad_embed"), (enc1.weight.grad, "grad_w1"), (enc2.weight.grad, "grad_w2")):
        assert got is not None, f"{what}: no gradient reached {key}"
        err = ((got.double().cpu() - torch.from_numpy(g[key]).double()).abs().max() / np.abs(g[key]).max()).item()
        print(f"{what} {key}: max |got - golden| / max|golden| = {err:.2e}")
        assert err < 5e-5, f"{what} {key}: {err:.2e}"


@pytest.mark.parametrize("cuda", [False, True])
@pytest.mark.parametrize("name", sorted(CASES))
def test_initializer_stack_matches_the_reference(name, cuda):
    g = load_golden(name)
    assert int(g["sigmoid1"]) == (CASES[name] == "node_degree")
    agg1, enc1, enc2, sets1 = build(g, CASES[name], cuda, None, None)
    l1 = [int(u) for u in g["layer1_nodes"]]
    with torch.no_grad():
        a1 = agg1.forward(l1, [sets1[u] for u in l1], None, initializer=CASES[name])
        assert a1.is_cuda == cuda
        assert_close_rowmax(a1.cpu(), g["agg1_out"], what=f"{name} agg1")
        assert_close_rowmax(enc1(torch.LongTensor(l1)).cpu(), g["enc1_out"], rows_dim=1, what=f"{name} enc1")
    _check_against_the_golden(g, agg1, enc1, enc2, cuda, name)


@pytest.mark.parametrize("cuda", [False, True])
@pytest.mark.parametrize("name", sorted(CASES))
def test_an_initializer_stack_with_a_fanout_takes_the_strict_path_not_the_engine(name, cuda):
    """A fanout above every set's size takes whole sets, so the reference's outputs still apply.  Without the initializer this
    stack is the two-hop engine's; with it only the aggregator's own forward expresses the lookup."""
    g = load_golden(name)
    agg1, enc1, enc2, _ = build(g, CASES[name], cuda, 12, 12)
    assert int(g["cnt1"].max()) < 12 and int(g["cnt2"].max()) < 12
    assert enc2._embed_detour() and enc1._embed_detour()
    _check_against_the_golden(g, agg1, enc1, enc2, cuda, f"{name} fanout 12")
    with torch.no_grad():
        assert_close_rowmax(enc2([int(s) for s in g["seeds"]]).cpu(), g["enc2_out"], rows_dim=1, what=f"{name} no grad")
    assert enc2._engine is None and enc1._engine is None


def test_a_stack_without_the_initializer_still_takes_the_engine():
    from test_gpu_forward import build_modules
    g = load_golden("tiny_gcn")
    sets1 = sets_from_padded(g["layer1_nodes"], g["nbr1"], g["cnt1"])
    sets2 = sets_from_padded(g["seeds"], g["nbr2"], g["cnt2"])
    enc1, enc2 = build_modules(g, int(g["k1"]), int(g["k2"]), False, sets1, sets2)
    assert not enc2._embed_detour()
    with torch.no_grad():
        out = enc2([int(s) for s in g["seeds"]])
    assert enc2._engine is not None and enc2._engine.generation == 1
    assert_close_rowmax(out, g["enc2_out"], rows_dim=1, what="tiny_gcn through the engine")


@pytest.mark.parametrize("name", sorted(CASES))
def test_a_feature_row_without_a_one_is_refused(name):
    g = load_golden(name)
    table = full_table(g)
    victim = int(g["nbr1"][0, 0])
    table[victim] = 0.0
    table[victim, 0] = 0.5
    _, enc1, _, _ = build(g, CASES[name], False, None, None, table=table)
    with pytest.raises(native.SageError):
        enc1([int(g["layer1_nodes"][0])])
