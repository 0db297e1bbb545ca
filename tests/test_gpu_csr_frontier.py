"""sage_csr_frontier on the MI355X: the distinct ids among a seed batch and all its neighbours, and the id -> row map, against the
numpy union -- on a graph with rows at every edge of the chunk split, one hub that names every node, and a pool of 70 nodes that
600 rows all name (contention on the same words of the map)."""
import numpy as np
import pytest
import torch

from sage355 import native, ops

pytestmark = pytest.mark.gpu
E = native.CSR_MEAN_CHUNK
N = 4096
SPECIAL = {0: 0, 1: 1, 2: 63, 3: 64, 4: 65, 5: E - 1, 6: E, 7: E + 1, 8: 2 * E + 1, 9: 3 * E + 1}     # node -> degree
HUB, ISOLATED = 10, 0
POOL = np.arange(100, 170)
POOL_ROWS = np.arange(200, 800)
SELF_LOOPS = (3, 7, 9, 20, 21, 22, 300, 301)


def build_graph(seed=0):
    """Rows of degree 0, 1, 63, 64, 65, 511, 512, 513, 1025, 1537; the hub is adjacent to every node (itself included); rows 200..799
    each name the whole pool, in an order of their own; the rest have 0..6 random neighbours.  Self loops on SELF_LOOPS (and the hub) only."""
    rng = np.random.default_rng(seed)
    deg = rng.integers(0, 7, N)
    for v, d in SPECIAL.items():
        deg[v] = d
    deg[HUB] = N
    deg[POOL_ROWS] = POOL.size
    rowptr = np.zeros(N + 1, dtype=np.int64)
    np.cumsum(deg, out=rowptr[1:])
    col = rng.integers(0, N, int(rowptr[-1])).astype(np.int32)
    for v in range(N):                                            # no accidental self loops
        row = col[rowptr[v]:rowptr[v + 1]]
        row[row == v] = (v + 1) % N
    col[rowptr[HUB]:rowptr[HUB + 1]] = rng.permutation(N)
    for v in POOL_ROWS:
        col[rowptr[v]:rowptr[v + 1]] = rng.permutation(POOL)
    for v in SELF_LOOPS:
        if deg[v] > 0:
            col[rowptr[v] + (deg[v] // 2)] = v
    return rowptr, col


ROWPTR, COL = build_graph()


@pytest.fixture(scope="module")
def graph():
    rowptr, col = ROWPTR, COL
    assert np.diff(rowptr)[[0, 1, 2, 3, 4, 5, 6, 7, 8, 9]].tolist() == [0, 1, 63, 64, 65, 511, 512, 513, 1025, 1537]
    return rowptr, col, torch.from_numpy(rowptr).cuda(), torch.from_numpy(col).cuda()


def union(rowptr, col, seeds):
    ids = set()
    for v in seeds:
        if 0 <= v < N:
            ids.add(int(v))
            ids.update(col[rowptr[v]:rowptr[v + 1]].tolist())
    return ids


def run(graph, seeds, fr=None, first_row=0, max_edges=None):
    """One insert into a frontier whose first free row is first_row; -> (frontier, count, nodes_out, pos) with the last three on the host."""
    _, _, rp, cl = graph
    if fr is None:
        fr = ops.CsrFrontier(N, "cuda", max_nodes=N + first_row)     # the caller's rows below first_row are room of their own
    if first_row:
        fr.clear(first_row)
    ops.csr_frontier(rp, cl, torch.as_tensor(np.asarray(seeds, dtype=np.int32)).cuda(), fr, max_edges=max_edges)
    torch.cuda.synchronize()
    return fr, fr.size(), fr.nodes.cpu().numpy(), fr.pos.cpu().numpy()


def check(graph, seeds, first_row=0, **kw):
    rowptr, col = graph[:2]
    fr, count, nodes, pos = run(graph, seeds, first_row=first_row, **kw)
    want = union(rowptr, col, seeds)
    got = nodes[first_row:count]
    assert count == first_row + len(want), (count, first_row, len(want))
    assert len(set(got.tolist())) == got.size, "an id appears twice in nodes_out"
    assert set(got.tolist()) == want
    assert np.array_equal(pos[got], np.arange(first_row, count)), "pos is not the inverse of nodes_out"
    rest = np.ones(N, dtype=bool)
    rest[got] = False
    assert (pos[rest] == -1).all(), "pos changed outside the set"
    assert (nodes[:first_row] == -1).all() and (nodes[count:] == -1).all(), "nodes_out written outside [first row, count)"
    fr.clear()
    torch.cuda.synchronize()
    assert (fr.pos.cpu().numpy() == -1).all() and fr.size() == 0, "clear left rows in the map"
    return fr, want


LONG = [5, 6, 7, 8, 9]
CASES = {
    "single": [33],
    "hub": [HUB],
    "isolated": [ISOLATED],
    "repeated": [7, 7, 33, 7, 8, 33, 8, 8, 250, 250],
    "mutual": [3] + COL[ROWPTR[3]:ROWPTR[4]].tolist()[:20],       # node 3 and 20 of its neighbours
    "pool_rows": POOL_ROWS.tolist(),
    "edges_of_the_split": list(SPECIAL),
    "all": list(range(N)),
    "out_of_range": [-1, 5, N, 250, -7, N + 5, 2 ** 31 - 1, 9, -(2 ** 31)],
}


@pytest.mark.parametrize("name", list(CASES))
def test_the_set_and_its_map_against_the_numpy_union(graph, name):
    check(graph, CASES[name])


def test_no_seeds_leaves_everything_as_it_was(graph):
    fr, count, nodes, pos = run(graph, [])
    assert count == 0 and (pos == -1).all() and (nodes == -1).all()


@pytest.mark.parametrize("seeds", ["edges_of_the_split", "all"])
def test_count_starting_above_zero(graph, seeds):
    check(graph, CASES[seeds], first_row=5)


@pytest.mark.parametrize("max_edges", [0, E + 1, 2 * E + 2])
def test_a_bound_that_is_too_small_gives_the_same_set(graph, max_edges):
    """max_edges = 0: no item list at all, every long row is walked by its own wave; the other two leave room for the chunks of the
    first long rows only."""
    check(graph, LONG + [HUB, 33, 250], max_edges=max_edges)


def test_a_reused_frontier_and_a_second_call_give_the_same_set(graph):
    fr, want = check(graph, CASES["pool_rows"])
    for seeds in (CASES["hub"], CASES["pool_rows"]):
        _, count, nodes, pos = run(graph, seeds, fr=fr)
        assert set(nodes[:count].tolist()) == union(graph[0], graph[1], seeds) and np.array_equal(pos[nodes[:count]], np.arange(count))
        fr.clear()
    torch.cuda.synchronize()
    assert (fr.pos.cpu().numpy() == -1).all()


def test_one_row_short_counts_on_and_writes_nothing_past_max_nodes(graph):
    rowptr, col, rp, cl = graph
    seeds = LONG + [33, 250]
    want = union(rowptr, col, seeds)
    fr = ops.CsrFrontier(N, "cuda", max_nodes=len(want) + 64)
    fr.nodes.fill_(-7)                                            # the sentinel
    fr.max_nodes = len(want) - 1
    ops.csr_frontier(rp, cl, torch.tensor(seeds, dtype=torch.int32).cuda(), fr)
    torch.cuda.synchronize()
    nodes = fr.nodes.cpu().numpy()
    assert fr.size() == len(want), "count must keep counting past max_nodes"
    assert (nodes[len(want) - 1:] == -7).all(), "a row at or past max_nodes was stored"
    kept = nodes[: len(want) - 1]
    assert len(set(kept.tolist())) == kept.size and set(kept.tolist()) < want
    with pytest.raises(native.SageError):
        fr.node_list()
    fr.refill()
    assert (fr.pos.cpu().numpy() == -1).all() and fr.size() == 0
