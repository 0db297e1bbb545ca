#!/usr/bin/env python3
"""Golden vectors of the reference's 1hot / node_degree initializers, made by IMPORTING THE REFERENCE (runs only where
the reference checkout is mounted, as make_golden.py does; the reference never travels).

    python tests/golden/make_golden_initializers.py     # rewrites tests/golden/tiny_1hot.npz and tiny_node_degree.npz

With these initializers the feature table holds one-hot rows that only INDEX a trainable nn.Embedding kept by the layer-1
aggregator (graphsage/aggregators.py:30-31, 68-71): row v for 1hot, the row of v's degree for node_degree (model.py:153-157),
and layer 1 applies a sigmoid for node_degree (encoders.py:58).  The stack is wired as run_model wires it (model.py:214-222):
gcn=True encoders over gcn=False aggregators, the initializer given to the layer-1 aggregator and encoder only.  Neighbour
sets are injected through num_sample=None (aggregators.py:47-48), so no random stream is involved.  The embedding's width
differs from the one-hot's on purpose: the reference's run_model makes them equal only because its loader hands the one-hot
in as the feature table.

Laid out like tiny_gcn.npz (make_golden.py), plus `embed` (the embedding's weight) and `grad_embed` (the reference's autograd's
gradient of it).  Only data is written: ids, neighbour lists, one-hot rows, weights, outputs, gradients.
"""
import os
import random
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
warnings.filterwarnings("ignore")

import make_golden as mg  # noqa: E402  (puts the reference's `graphsage` first on sys.path and imports its classes)
from make_golden import Encoder, MeanAggregator, G, pad_sets, presample, quiet, xavier  # noqa: E402

EMBED_DIM, H1, H2, K1, K2 = 7, 6, 5, 4, 3


def graph():
    """30 nodes: a hub (node 0, degree 12), a ring over 1..24 with chords, a pendant chain 25-26-27, a pair 28-29 hanging off the
    hub ... and node 17 cut out of everything (isolated: degree 0)."""
    edges = [(0, v) for v in (1, 3, 5, 8, 11, 14, 16, 19, 22, 24, 28, 29)]
    ring = [v for v in range(1, 25) if v != 17]
    edges += list(zip(ring, ring[1:] + ring[:1]))
    edges += [(2, 9), (4, 13), (6, 20), (10, 21), (12, 23), (7, 15), (24, 25), (25, 26), (26, 27), (28, 29)]
    src, dst = zip(*edges)
    g = G.csr_from_edges(src, dst, 30, symmetric=True)
    assert int(g.degrees()[17]) == 0 and int(g.degrees().max()) == 12
    return g


def case(name, initializer, seed):
    g = graph()
    n = g.num_nodes
    adj = g.to_adj_lists()
    deg = g.degrees()
    if initializer == "1hot":
        index, rows = np.arange(n), n
    else:
        index, rows = deg.astype(np.int64), int(deg.max()) + 1            # model.py:153-157
    table = torch.zeros(n, rows)
    table[torch.arange(n), torch.from_numpy(index)] = 1.0
    assert EMBED_DIM != rows

    rng = random.Random(seed)
    gen = torch.Generator().manual_seed(seed)
    seeds = [v for v in range(n) if deg[v] > 0][::2]
    sets2 = presample(adj, seeds, K2, rng)
    layer1_nodes = sorted(set().union(*sets2.values()))
    sets1 = presample(adj, layer1_nodes, K1, rng)
    w1 = xavier((H1, EMBED_DIM), gen)
    w2 = xavier((H2, H1), gen)
    embed = torch.randn(rows, EMBED_DIM, generator=gen)

    features = torch.nn.Embedding(n, rows)
    features.weight = torch.nn.Parameter(table.clone(), requires_grad=False)
    agg1 = MeanAggregator(features, cuda=False, feature_dim=EMBED_DIM, num_nodes=rows, initializer=initializer)
    enc1 = quiet(Encoder, features, EMBED_DIM, H1, sets1, agg1, num_sample=None, gcn=True, cuda=False, initializer=initializer)
    agg2 = MeanAggregator(lambda nodes: enc1(nodes).t(), cuda=False)
    enc2 = quiet(Encoder, lambda nodes: enc1(nodes).t(), enc1.embed_dim, H2, sets2, agg2, num_sample=None, base_model=enc1, gcn=True,
                 cuda=False)
    with torch.no_grad():
        enc1.weight.copy_(w1)
        enc2.weight.copy_(w2)
        agg1.embed.weight.copy_(embed)
        agg1_out = agg1.forward(layer1_nodes, [sets1[u] for u in layer1_nodes], None, initializer=initializer)
        enc1_out = enc1(torch.LongTensor(layer1_nodes))
        agg2_out = agg2.forward(seeds, [sets2[s] for s in seeds], None)
        enc2_out = enc2(seeds)
    cot = torch.randn(enc2_out.shape, generator=gen)
    (enc2(seeds) * cot).sum().backward()
    grad_embed = agg1.embed.weight.grad
    assert grad_embed is not None and float(grad_embed.abs().max()) > 0

    nbr2, cnt2 = pad_sets(seeds, sets2, K2)
    nbr1, cnt1 = pad_sets(layer1_nodes, sets1, K1)
    touched = sorted(set(layer1_nodes) | set(int(x) for x in nbr1[nbr1 >= 0]))
    np.savez_compressed(
        os.path.join(HERE, name + ".npz"),
        num_nodes=np.int64(n), d0=np.int64(rows), embed_dim=np.int64(EMBED_DIM), k1=np.int64(K1), k2=np.int64(K2), gcn=np.int64(1),
        sigmoid1=np.int64(initializer == "node_degree"), sigmoid2=np.int64(0), node_degree=np.int64(initializer == "node_degree"),
        seeds=np.array(seeds, dtype=np.int64), nbr2=nbr2, cnt2=cnt2, layer1_nodes=np.array(layer1_nodes, dtype=np.int64), nbr1=nbr1, cnt1=cnt1,
        feat_ids=np.array(touched, dtype=np.int64), feat_rows=table[touched].numpy(),
        w1=w1.numpy(), w2=w2.numpy(), embed=embed.numpy(), agg1_out=agg1_out.numpy(), enc1_out=enc1_out.numpy(), agg2_out=agg2_out.numpy(),
        enc2_out=enc2_out.numpy(), cotangent=cot.numpy(), grad_w1=enc1.weight.grad.numpy(), grad_w2=enc2.weight.grad.numpy(),
        grad_embed=grad_embed.numpy())
    print(f"{name}: B={len(seeds)} |S1|={len(layer1_nodes)} rows={rows} embed {tuple(embed.shape)} enc2_out {tuple(enc2_out.shape)} "
          f"max|grad_embed|={float(grad_embed.abs().max()):.4f} rows with gradient {int((grad_embed.abs().sum(1) > 0).sum())}")


if __name__ == "__main__":
    assert mg.REF in sys.path[0]
    case("tiny_1hot", "1hot", 21)
    case("tiny_node_degree", "node_degree", 22)
