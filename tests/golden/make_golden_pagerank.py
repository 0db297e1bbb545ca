#!/usr/bin/env python3
"""Golden vectors of the `pagerank` initializer, made by CALLING networkx as the reference does (model.py:158-162:
nx.pagerank(G) with its defaults; runs only where networkx is installed -- the tests need only the .npz).

    python tests/golden/make_golden_pagerank.py     # rewrites tests/golden/pagerank_cases.npz

Only data is written.  For every case <c> in `cases`: <c>_rowptr (int64), <c>_col (int32) -- the CSR, each row the sorted
neighbours (out-neighbours for a directed case) of its node, a self loop one entry --, <c>_symmetric, <c>_x (float64, networkx's
result), <c>_iterations (the step after which the fp64 restatement below stops, which is where networkx stops) and <c>_err (the
restatement's err of the last two steps).

Cases:
  a  the 30-node graph of make_golden_initializers.py: a hub of degree 12, isolated node 17
  b  1500 nodes: node 0 with 1100 random neighbours, node 1 with 513, node 2 with 65 (rows on both sides of the 512-entry chunk
     and of a 64-entry trip), 3000 edges whose second endpoint is power-law distributed (n * u^2.5), self loops on 0, 5 and 6, the
     last 40 nodes isolated
  c  the same recipe at 2100 nodes, another seed, no self loops
  d  a small DIRECTED graph with a sink (and a node nobody links to), built as an nx.DiGraph: rows are out-edge lists

Two conditions are asserted, so that the fixture can carry an fp32 implementation: the fp64 restatement matches networkx to 1e-12
relative, and the stopping step is clear of the threshold (err_last <= 0.99 N tol, err_prev >= 1.01 N tol) -- an fp32 err cannot
fall on the other side of it.
"""
import os

import networkx as nx
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ALPHA, TOL, MAX_ITER = 0.85, 1e-6, 100


def restatement(rowptr, col, alpha=ALPHA, tol=TOL, max_iter=MAX_ITER):
    """nx.pagerank's power iteration with its defaults in fp64 numpy over out-edge lists (for a symmetric graph: its CSR).
    -> (x, iterations, [err of every step])."""
    n = len(rowptr) - 1
    deg = np.diff(rowptr)
    src = np.repeat(np.arange(n), deg)
    inv_out = np.where(deg > 0, 1.0 / np.maximum(deg, 1), 0.0)
    x = np.full(n, 1.0 / n)
    errs = []
    for it in range(1, max_iter + 1):
        s = np.bincount(col, weights=(x * inv_out)[src], minlength=n)
        mass = x[deg == 0].sum()
        x_next = alpha * (s + mass / n) + (1.0 - alpha) / n
        errs.append(np.abs(x_next - x).sum())
        x = x_next
        if errs[-1] < n * tol:
            return x, it, errs
    raise RuntimeError("no convergence")


def hub_graph():
    edges = [(0, v) for v in (1, 3, 5, 8, 11, 14, 16, 19, 22, 24, 28, 29)]
    ring = [v for v in range(1, 25) if v != 17]
    edges += list(zip(ring, ring[1:] + ring[:1]))
    edges += [(2, 9), (4, 13), (6, 20), (10, 21), (12, 23), (7, 15), (24, 25), (25, 26), (26, 27), (28, 29)]
    g = nx.Graph()
    g.add_nodes_from(range(30))
    g.add_edges_from(edges)
    assert g.degree(17) == 0 and g.degree(0) == 12
    return g


def skewed_graph(n, seed, self_loops):
    rng = np.random.default_rng(seed)
    live = n - 40
    g = nx.Graph()
    g.add_nodes_from(range(n))
    for hub, k in ((0, 1100), (1, 513), (2, 65)):
        others = np.setdiff1d(np.arange(live), [hub])
        g.add_edges_from((hub, int(v)) for v in rng.choice(others, k, replace=False))
    a = rng.integers(0, live, 3000)
    b = np.minimum((live * rng.random(3000) ** 2.5).astype(np.int64), live - 1)
    g.add_edges_from((int(u), int(v)) for u, v in zip(a, b) if u != v)
    g.add_edges_from((v, v) for v in self_loops)
    assert all(g.degree(v) == 0 for v in range(live, n))
    return g


def directed_graph():
    """14 nodes: a cycle 0..9 with chords, 10 -> 11 -> 12 where 12 is a sink (no out-edges), 13 links out and nobody links to it."""
    g = nx.DiGraph()
    g.add_nodes_from(range(14))
    g.add_edges_from((v, (v + 1) % 10) for v in range(10))
    g.add_edges_from([(0, 5), (3, 7), (7, 2), (9, 4), (4, 10), (10, 11), (11, 12), (6, 12), (13, 0), (13, 8), (2, 2)])
    assert g.out_degree(12) == 0 and g.in_degree(13) == 0
    return g


def csr(g):
    n = g.number_of_nodes()
    rows = [sorted(g[v]) for v in range(n)]
    rowptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum([len(r) for r in rows], out=rowptr[1:])
    return rowptr, np.array([u for r in rows for u in r], dtype=np.int32)


def main():
    out, names = {}, []
    for name, g in (("a", hub_graph()), ("b", skewed_graph(1500, 0, (0, 5, 6))), ("c", skewed_graph(2100, 3, ())), ("d", directed_graph())):
        pr = nx.pagerank(g)
        n = g.number_of_nodes()
        ref = np.array([pr[v] for v in range(n)])
        rowptr, col = csr(g)
        x, it, errs = restatement(rowptr, col)
        rel = float((np.abs(x - ref) / ref).max())
        thr = n * TOL
        assert rel <= 1e-12, (name, rel)
        assert errs[-1] <= 0.99 * thr and errs[-2] >= 1.01 * thr, (name, errs[-1] / thr, errs[-2] / thr)
        names.append(name)
        out.update({f"{name}_rowptr": rowptr, f"{name}_col": col, f"{name}_symmetric": np.int64(not g.is_directed()), f"{name}_x": ref,
                    f"{name}_iterations": np.int64(it), f"{name}_err": np.array(errs[-2:])})
        print(f"{name}: N={n} entries={len(col)} max row={int(np.diff(rowptr).max())} iterations={it} err_last/thr={errs[-1] / thr:.3f} "
              f"err_prev/thr={errs[-2] / thr:.3f} restatement vs networkx {rel:.1e}")
    np.savez_compressed(os.path.join(HERE, "pagerank_cases.npz"), cases=np.array(names), **out)


if __name__ == "__main__":
    main()
