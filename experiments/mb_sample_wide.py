"""Wide sampler (sage_sample_neighbors_wide) and the operator-level two-hop forward on the config-3 R-MAT (2^20 nodes, 16 M edge draws):
median of 20 calls, device events around a call that ends in a synchronise (so launch and host time of the call are inside).

  python experiments/mb_sample_wide.py [--python-reps 20]

Prints one line per figure ("Fanouts above 64", quotes them):
  * sample_neighbors_wide at (n, k) = (23 000, 128) and (4096, 1024), no frontier;
  * the narrow kernel at (23 000, 64) and the wide one on the same call, alternating in one process;
  * one two_hop_forward at B = 256, k = 100 / 100 (gcn encoder, 256 -> 128 -> 128);
  * the same stack through Encoder.forward with the routing the tree had BEFORE the wide sampler (native.MAX_FANOUT_WIDE lowered to
    native.MAX_FANOUT for that measurement: both layers fall through to _forward_generic, random.sample per node on the host).
"""
import argparse
import os
import random
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "graphsage-simple_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from sage355 import native, ops  # noqa: E402
from sage355.aggregators import MeanAggregator  # noqa: E402
from sage355.encoders import Encoder  # noqa: E402
from sage355.graph import rmat_graph  # noqa: E402
from sage355.twohop_ops import two_hop_forward  # noqa: E402

DEV = "cuda"


def timed(fn):
    """One call, in microseconds: device events around it, the call's work finished before the second event is read."""
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1e3


def median_us(fn, reps=20, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    return statistics.median(timed(fn) for _ in range(reps))


class CsrAdjacency(dict):
    """adj_lists[v] as a set, built from the CSR on first use (the strict path reads only the rows it visits)."""

    def __init__(self, g):
        super().__init__()
        self.g = g

    def __missing__(self, v):
        s = self[v] = set(self.g.neighbors(int(v)).tolist())
        return s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--python-reps", type=int, default=20)
    args = ap.parse_args()
    g = rmat_graph(20, 16_000_000, seed=0)
    rowptr, col = g.to(DEV)
    deg = g.degrees()
    cands = np.nonzero(deg > 0)[0]
    rng = np.random.default_rng(0)
    print(f"graph: {g.num_nodes} nodes, {g.col.size} directed edges, {(deg > 64).sum()} nodes above 64 neighbours, "
          f"{(deg > 128).sum()} above 128, {(deg > 1024).sum()} above 1024")

    def sampler(fn, n, k):
        nodes = torch.from_numpy(rng.choice(cands, n, replace=False).astype(np.int32)).to(DEV)
        nbr = torch.empty((n, k), dtype=torch.int32, device=DEV)
        cnt = torch.empty(n, dtype=torch.int32, device=DEV)
        return lambda: fn(rowptr, col, nodes, k, 1, ops.TAG_INNER, out_nbr=nbr, out_cnt=cnt)

    print(f"sample_neighbors_wide n=23000 k=128: {median_us(sampler(ops.sample_neighbors_wide, 23_000, 128)):.1f} us")
    print(f"sample_neighbors_wide n=4096 k=1024: {median_us(sampler(ops.sample_neighbors_wide, 4096, 1024)):.1f} us")
    # narrow and wide kernel on the same call, alternating
    nodes = torch.from_numpy(rng.choice(cands, 23_000, replace=False).astype(np.int32)).to(DEV)
    nbr = torch.empty((23_000, 64), dtype=torch.int32, device=DEV)
    cnt = torch.empty(23_000, dtype=torch.int32, device=DEV)
    calls = {name: (lambda fn=fn: fn(rowptr, col, nodes, 64, 1, ops.TAG_INNER, out_nbr=nbr, out_cnt=cnt))
             for name, fn in (("sample_neighbors", ops.sample_neighbors), ("sample_neighbors_wide", ops.sample_neighbors_wide))}
    for fn in calls.values():
        for _ in range(3):
            fn()
    times = {name: [] for name in calls}
    for _ in range(20):
        for name, fn in calls.items():
            times[name].append(timed(fn))
    for name, t in times.items():
        print(f"{name} n=23000 k=64 (alternating): {statistics.median(t):.1f} us")

    # the two-layer stack at B = 256, fanouts 100 / 100
    d0, h1, h2, b, k = 256, 128, 128, 256, 100
    gen = torch.Generator().manual_seed(0)
    table = torch.randn(g.num_nodes, d0, generator=gen)
    table_d = table.to(DEV)
    w1, w2 = torch.randn(h1, d0, generator=gen) / 16, torch.randn(h2, h1, generator=gen) / 11
    w1_d, w2_d = w1.to(DEV), w2.to(DEV)
    seeds = rng.choice(cands, b, replace=False).astype(np.int32)
    seeds_d = torch.from_numpy(seeds).to(DEV)
    with torch.no_grad():
        _, sets = two_hop_forward(rowptr, col, table_d, w1_d, w2_d, seeds_d, k, k, 7, return_sets=True)
        print(f"two_hop_forward B={b} k={k}/{k}: layer-1 rows {sets['n_s1']}, sampled ids {int(sets['cnt1'].sum())}")
        t = median_us(lambda: two_hop_forward(rowptr, col, table_d, w1_d, w2_d, seeds_d, k, k, random.getrandbits(64)))
        print(f"two_hop_forward B={b} k={k}/{k} (operators, device sampler): {t:.1f} us")

        # the Encoder stack as it was routed before: the strict path on the host
        adj = CsrAdjacency(g)
        features = torch.nn.Embedding(g.num_nodes, d0, _weight=table)        # cuda=False: model.py's default, ids and sets stay on the host
        features.weight.requires_grad = False
        agg1 = MeanAggregator(features, cuda=False)
        enc1 = Encoder(features, d0, h1, adj, agg1, num_sample=k, gcn=True, cuda=False)
        agg2 = MeanAggregator(lambda ids: enc1(ids).t(), cuda=False)
        enc2 = Encoder(lambda ids: enc1(ids).t(), h1, h2, adj, agg2, num_sample=k, base_model=enc1, gcn=True, cuda=False)
        enc1.weight.data, enc2.weight.data = w1.clone(), w2.clone()
        wide = native.MAX_FANOUT_WIDE
        native.MAX_FANOUT_WIDE = native.MAX_FANOUT
        try:
            assert not enc2._can_two_hop_ops() and not enc2._can_fuse_two_hop()
            seed_list = [int(s) for s in seeds]
            t = median_us(lambda: enc2(seed_list), reps=args.python_reps, warmup=1)
        finally:
            native.MAX_FANOUT_WIDE = wide
        print(f"Encoder stack B={b} k={k}/{k}, previous routing (random.sample per node on the host), median of {args.python_reps}: {t:.1f} us")


if __name__ == "__main__":
    main()
