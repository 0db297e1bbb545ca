#!/usr/bin/env python3
"""Golden vectors of the `eigen_decomposition` initializer, made by CALLING numpy as the reference does (model.py:163-180:
w, v = LA.eig(nx.to_numpy_array(G)), eigenvalues sorted descending, column j of the table the eigenvector of the j-th largest;
runs only where networkx is installed -- the tests need only the .npz files).

    python tests/golden/make_golden_eigen.py     # rewrites tests/golden/eigen_cases.npz and eigen_cases_cora_<i>.npz

Only data is written.  eigen_cases.npz holds `cases` and for every case <c>: <c>_graph (where its CSR lives), <c>_k, <c>_values
(float64 [k + 1]: the k + 1 largest eigenvalues, descending) and -- except for the Cora case -- <c>_rowptr (int64), <c>_col (int32)
and <c>_vectors (float64 [N, k]: the eigenvectors of the k largest, in LAPACK's signs).  The Cora case's CSR is
cora_topology.npz; its 2708 x 100 fp64 vectors are over a megabyte, so they are cut by columns into eigen_cases_cora_0.npz,
_1, _2 (`vectors`: float64 [N, <= 34], `first`: the first column's index), each below the size limit of a committed file.

Cases:
  a     case a of make_golden_pagerank.py (30 nodes, a hub, an isolated node), k = 4
  b     its case b (1500 nodes, rows of 1143, 514 and 66 entries, self loops, 40 isolated nodes), k = 8
  b32   the same graph, k = 32
  c     its case c (2100 nodes, no self loops), k = 16
  cora  the Cora topology (2708 nodes), k = 100
The graphs of a, b and c are read from pagerank_cases.npz (the CSR that script wrote) and rebuilt as nx.Graph.

Asserted for every case, because tests/test_gpu_eigen.py relies on it (TOL = 3e-5 is the tolerance the GPU tests run at):
  * LA.eig's eigenvalues are real (imaginary parts at rounding level occur only inside the cluster at 0) and match eigh's to
    1e-10; its top-k eigenvectors are real and satisfy A v = lambda v to 1e-10
  * lambda_k - lambda_(k+1) >= 2 sqrt(k) TOL lambda_1: a run that misses one of the top k pairs shows as a violation
  * lambda_k > 0
"""
import os

import networkx as nx
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TOL = 3e-5
CASES = (("a", "a", 4), ("b", "b", 8), ("b32", "b", 32), ("c", "c", 16), ("cora", "cora", 100))
CORA_PART = 34                                                       # columns per file: 2708 * 34 * 8 bytes = 0.70 MiB


def graph_of(rowptr, col):
    n = len(rowptr) - 1
    g = nx.Graph()
    g.add_nodes_from(range(n))
    g.add_edges_from((int(u), int(v)) for u in range(n) for v in col[rowptr[u]:rowptr[u + 1]])
    return g


def top_pairs(g, k):
    """The reference's computation: LA.eig of the dense adjacency matrix, sorted descending -> (k + 1 values, k vectors)."""
    a = nx.to_numpy_array(g, nodelist=range(g.number_of_nodes()))
    assert np.array_equal(a, a.T)
    w, v = np.linalg.eig(a)
    assert float(np.abs(np.imag(w)).max()) <= 1e-10                  # rounding-level pairs inside the cluster at 0 only
    order = np.argsort(-np.real(w), kind="stable")
    w, v = np.real(w)[order], v[:, order[:k]]
    assert float(np.abs(np.imag(v)).max()) == 0.0
    v = np.real(v)
    assert float(np.abs(w - np.linalg.eigvalsh(a)[::-1]).max()) <= 1e-10
    v = v / np.linalg.norm(v, axis=0)
    assert float(np.abs(a @ v - v * w[:k]).max()) <= 1e-10
    return w[:k + 1].copy(), np.ascontiguousarray(v)


def main():
    pr = np.load(os.path.join(HERE, "pagerank_cases.npz"))
    cora = np.load(os.path.join(HERE, "cora_topology.npz"))
    csrs = {c: (pr[f"{c}_rowptr"].astype(np.int64), pr[f"{c}_col"].astype(np.int32)) for c in "abc"}
    csrs["cora"] = (cora["rowptr"].astype(np.int64), cora["col"].astype(np.int32))
    out, names = {}, []
    for name, graph, k in CASES:
        rowptr, col = csrs[graph]
        w, v = top_pairs(graph_of(rowptr, col), k)
        gap, need = w[k - 1] - w[k], 2 * np.sqrt(k) * TOL * w[0]
        assert gap >= need, (name, gap, need)
        assert w[k - 1] > 0, (name, w[k - 1])
        names.append(name)
        out.update({f"{name}_graph": np.array(graph), f"{name}_k": np.int64(k), f"{name}_values": w})
        if graph == "cora":
            for i, first in enumerate(range(0, k, CORA_PART)):
                np.savez_compressed(os.path.join(HERE, f"eigen_cases_cora_{i}.npz"), first=np.int64(first),
                                    vectors=np.ascontiguousarray(v[:, first:first + CORA_PART]))
        else:
            out.update({f"{name}_rowptr": rowptr, f"{name}_col": col, f"{name}_vectors": v})
        print(f"{name}: N={len(rowptr) - 1} entries={len(col)} k={k} lambda_1={w[0]:.6f} lambda_k={w[k - 1]:.6f} "
              f"gap/lambda_1={gap / w[0]:.4f} (needed {need / w[0]:.5f}: margin {gap / need:.2f}x)")
    np.savez_compressed(os.path.join(HERE, "eigen_cases.npz"), cases=np.array(names), **out)


if __name__ == "__main__":
    main()
