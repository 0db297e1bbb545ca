"""Stand-in node-classification data on a REAL citation topology.

The reference's feature/label files (cora/cora.content, pubmed-data/*.NODE.paper.tab) are not in
the mount, so F1 comparisons run on "real topology + synthesised content":
labels = graph-Voronoi cells around random centres (so they correlate with the topology, as topics
do in a citation graph), features = sparse bag-of-words drawn mostly from the label's topic words.
Deterministic in (graph, seed); used identically by tests/golden/make_golden.py (which trains the
REFERENCE on it) and by the GPU training test.
"""
import numpy as np


def graph_voronoi_labels(graph, num_classes, rng):
    n = graph.num_nodes
    labels = np.full(n, -1, dtype=np.int64)
    order = rng.permutation(n)
    centres = order[:num_classes]
    labels[centres] = np.arange(num_classes)
    frontier = list(centres)
    while frontier:
        nxt = []
        for v in frontier:
            for u in graph.neighbors(v):
                if labels[u] < 0:
                    labels[u] = labels[v]
                    nxt.append(int(u))
        frontier = nxt
    missing = labels < 0
    labels[missing] = rng.integers(0, num_classes, size=int(missing.sum()))
    return labels


def pagerank_table(graph, device, **kw):
    """float32 [N, 1] on `device`: the frozen feature table of --initializer pagerank (model.py:159-162: nx.pagerank(G) as the
    single feature column), computed on the device by ops.pagerank; **kw are its keywords (alpha, tol, max_iter, symmetric).  Layer 1
    of this initializer goes through a sigmoid (encoders.py:58): the trainers and run drivers take it as act1=ACT_SIGMOID."""
    from . import ops
    rowptr, col = graph.to(device)
    x, _ = ops.pagerank(rowptr, col, **kw)
    return x.reshape(-1, 1)


def eigen_table(graph, device, feature_dim=100, **kw):
    """float32 [N, feature_dim] on `device`: the frozen feature table of --initializer eigen_decomposition (model.py:163-180: column
    j is the eigenvector of the j-th largest eigenvalue of the adjacency matrix, a dense LA.eig there), computed on the device by
    ops.eigen_top; **kw are its keywords (tol, max_iter, degree, guard, seed, check_symmetric, history).  A column's sign is
    LAPACK's in the reference and ops.eigen_top's rule here (largest entry positive).  Layer 1 keeps the default ReLU: this
    initializer is not in encoders.py:58's sigmoid list."""
    from . import ops
    rowptr, col = graph.to(device)
    _, vectors, _ = ops.eigen_top(rowptr, col, feature_dim, **kw)
    return vectors


def standin_citation(graph, num_classes=7, feat_dim=1433, words_per_node=18, topic_words=60, purity=0.7, seed=0):
    """-> (feat_data float32 [N, feat_dim] 0/1, labels int64 [N, 1]) in the reference loaders' layout
    (model.py:267-269: feat_data, labels [N,1])."""
    rng = np.random.default_rng(seed)
    n = graph.num_nodes
    labels = graph_voronoi_labels(graph, num_classes, rng)
    topics = np.stack([rng.choice(feat_dim, topic_words, replace=False) for _ in range(num_classes)])
    feats = np.zeros((n, feat_dim), dtype=np.float32)
    from_topic = rng.random((n, words_per_node)) < purity
    topic_pick = topics[labels[:, None], rng.integers(0, topic_words, size=(n, words_per_node))]
    random_pick = rng.integers(0, feat_dim, size=(n, words_per_node))
    words = np.where(from_topic, topic_pick, random_pick)
    feats[np.arange(n)[:, None], words] = 1.0
    return feats, labels.reshape(-1, 1)
