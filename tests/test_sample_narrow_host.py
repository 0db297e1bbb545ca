"""CPU side of the narrow sampler's and the hash frontier's edge-shape tests (csrc/sage_sample.hip, sage_sample_body.h, sage_hash_insert and
sage_group_positions in sage_common.h): the case builders of test_gpu_sample_narrow.py, and the conditions those cases must meet, asserted
here from the reference sets alone so that the GPU tests cannot pass vacuously.

The reference of every expectation is test_sample_wide_host.wide_ref (ids outside the graph are empty rows), pinned to oracle/sampler_ref.c
there and, on these very graphs, below."""
import functools

import numpy as np
import pytest

from oracle import sampler_ref
from sage355 import native
from test_sample_wide_host import wide_ref

SEED = 0xC0FFEE1234
K_EDGE = [1, 2, 7, 8, 9, 16, 17, 32, 33, 63, 64]          # both sides of every lane-group switch (8 | 9, 16 | 17, 32 | 33) and the limits
N_EDGE = 515                                              # 8 lanes per node, 256-thread blocks: 17 blocks, the last one partial
FRONTIER_THREADS = 1024                                   # block size of the frontier variants unless SAGE_SO_THREADS says otherwise
FIXED_DEGREES = [0, 1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 5000, 70000]
POOL = 6000                                               # ids of every row but the hub's: small enough that rows share many ids
M32 = 0xFFFFFFFF


def lane_group(k):
    """Lanes per node of pick_by_fanout_t."""
    return 8 if k <= 8 else 16 if k <= 16 else 32 if k <= 32 else 64


def boundary_degrees(k):
    return FIXED_DEGREES + [max(k - 1, 0), k, k + 1, 2 * k + 3]


def narrow_edge_csr(k, n):
    """(rowptr, col, nodes): a CSR whose degrees sit on every boundary of the narrow sampler for fanout k (take-all / Floyd at k, the lane
    groups' widths, a row above 2^16 for the multiply-shift bound) with about 20 random ones between, rows of distinct ids drawn from a
    small pool (the 70 000-neighbour row from a wider range of its own), and n node ids in shuffled order: every node at least once,
    repeats, and num_nodes, num_nodes + 7, -1 and -5, which are outside the graph."""
    rng = np.random.default_rng(1000 + k)
    deg = np.array(boundary_degrees(k) + rng.integers(0, 3 * k + 1, 20).tolist(), dtype=np.int64)
    deg = deg[rng.permutation(deg.size)]
    num_nodes = deg.size
    assert n >= num_nodes + 4
    rowptr = np.zeros(num_nodes + 1, np.int64)
    rowptr[1:] = np.cumsum(deg)
    rows = [rng.choice(POOL, int(d), replace=False) if d <= POOL else POOL + rng.choice(4 * int(d), int(d), replace=False) for d in deg]
    rows[int(np.nonzero(deg == 1)[0][0])][:] = int(np.argmax(deg))      # a row that is always taken whole names a node of the list
    col = np.concatenate(rows).astype(np.int32)
    bad = [num_nodes, num_nodes + 7, -1, -5]
    nodes = np.concatenate([rng.permutation(num_nodes), rng.integers(0, num_nodes, n - num_nodes - len(bad)), bad]).astype(np.int32)
    return rowptr, col, nodes[rng.permutation(n)]


@functools.lru_cache(maxsize=None)
def edge_case(k, n=N_EDGE):
    """narrow_edge_csr(k, n), built once; the arrays are shared between tests and must not be written."""
    case = narrow_edge_csr(k, n)
    for a in case:
        a.setflags(write=False)
    return case


@functools.lru_cache(maxsize=None)
def edge_ref(k, tag, n=N_EDGE):
    """wide_ref on edge_case(k, n): (nbr, cnt), computed once and shared."""
    rowptr, col, nodes = edge_case(k, n)
    nbr, cnt = wide_ref(rowptr, col, nodes, k, SEED, tag)
    nbr.setflags(write=False)
    cnt.setflags(write=False)
    return nbr, cnt


def expected_frontier(nbr, cnt, nodes, insert_self):
    """The set a frontier must hold after these lists: the valid sampled ids, and with insert_self every non-negative node id."""
    valid = np.arange(nbr.shape[1])[None, :] < cnt[:, None]
    ids = set(nbr[valid].tolist())
    if insert_self:
        ids |= {int(v) for v in nodes if v >= 0}
    return ids


def hash_slot(ids, mask):
    """sage_hash_slot (csrc/sage_common.h) for an array of ids."""
    h = (np.asarray(ids, dtype=np.uint64) * np.uint64(0x9E3779B1)) & np.uint64(M32)
    h ^= h >> np.uint64(15)
    return (h & np.uint64(mask)).astype(np.int64)


def wrap_ids(capacity, count):
    """`count` distinct non-negative ids for a table of `capacity` slots whose probing must wrap past the last slot: two ids whose home
    is slot capacity - 2 (none when count < 4), two whose home is capacity - 1, then random ids up to 2^31 - 1.  In whatever order they
    are inserted, the ids of the last two slots overflow them into slot 0 and beyond."""
    assert capacity >= 4 and capacity & (capacity - 1) == 0 and count >= 2
    scan = np.arange(64 * capacity, dtype=np.int64)
    home = hash_slot(scan, capacity - 1)
    last, before = scan[home == capacity - 1], scan[home == capacity - 2]
    n_before = 2 if count >= 4 else 0
    head = np.concatenate([before[:n_before], last[:2]])
    rng = np.random.default_rng(capacity + count)
    rest = np.setdiff1d(np.unique(np.concatenate([rng.integers(0, 1 << 31, 2 * count), [(1 << 31) - 1]])), head)
    rest = rest[rng.permutation(rest.size)][:count - head.size]
    ids = np.concatenate([head, rest]).astype(np.int32)
    assert ids.size == count
    return ids


# ---------------------------------------------------------------------------------------------------------------- the builders' own conditions
@pytest.mark.parametrize("k", K_EDGE)
def test_edge_csr_has_every_boundary_degree_distinct_rows_and_the_ids_outside_the_graph(k):
    rowptr, col, nodes = edge_case(k)
    deg = np.diff(rowptr)
    num_nodes = deg.size
    assert set(boundary_degrees(k)) <= set(deg.tolist())
    assert {0, k, k + 1, 70000} <= set(deg.tolist()) and deg.max() > 1 << 16
    for v in range(num_nodes):
        row = col[rowptr[v]:rowptr[v + 1]]
        assert np.unique(row).size == row.size and (row >= 0).all()
    assert nodes.size == N_EDGE and nodes.dtype == np.int32
    assert set(range(num_nodes)) <= set(nodes.tolist())                                   # every node at least once
    assert {num_nodes, num_nodes + 7, -1, -5} <= set(nodes.tolist())
    assert np.bincount(nodes[(nodes >= 0) & (nodes < num_nodes)]).max() > 1               # repeats
    assert N_EDGE % (256 // 8) != 0 and -(-N_EDGE // (256 // 8)) == 17                    # k <= 8 without a frontier: a partial last block
    assert N_EDGE % (FRONTIER_THREADS // lane_group(k)) != 0                              # and with one, at every lane-group width


@pytest.mark.parametrize("k", K_EDGE)
def test_restatement_equals_the_c_oracle_on_the_edge_graphs(k):
    rowptr, col, nodes = edge_case(k)
    inside = (nodes >= 0) & (nodes < rowptr.size - 1)
    for tag in (native.TAG_INNER, native.TAG_OUTER):
        nbr, cnt = edge_ref(k, tag)
        want_nbr, want_cnt = sampler_ref.sample_neighbors(rowptr, col, nodes[inside], k, SEED, tag)
        assert np.array_equal(cnt[inside], want_cnt) and np.array_equal(nbr[inside], want_nbr)
        assert (cnt[~inside] == 0).all() and (nbr[~inside] == -1).all()
    deg = np.diff(rowptr)
    floyd = np.where(inside, deg[np.clip(nodes, 0, deg.size - 1)], 0) > k                  # rows that are drawn, not taken whole
    assert floyd.any() and not np.array_equal(edge_ref(k, native.TAG_INNER)[0][floyd], edge_ref(k, native.TAG_OUTER)[0][floyd])


@pytest.mark.parametrize("k", K_EDGE)
def test_edge_lists_repeat_ids_across_blocks_inside_blocks_and_among_the_nodes(k):
    """What makes the frontier tests bite, from the reference sets alone, with the default 1024-thread blocks (1024 / G nodes each)."""
    _, _, nodes = edge_case(k)
    nbr, cnt = edge_ref(k, native.TAG_OUTER)
    per_block = FRONTIER_THREADS // lane_group(k)
    blocks_of, rows_in_block = {}, {}
    for r in range(nodes.size):
        for x in nbr[r, :cnt[r]].tolist():
            blocks_of.setdefault(x, set()).add(r // per_block)
            key = (x, r // per_block)
            rows_in_block[key] = rows_in_block.get(key, 0) + 1
    assert max(len(b) for b in blocks_of.values()) >= 4            # the same id from many blocks: the global compare-and-swap
    assert max(rows_in_block.values()) >= 2                        # and from several nodes of one block: the LDS dedupe
    assert set(blocks_of) & set(nodes.tolist())                    # a sampled id is a node of the list: the insert_self union is not disjoint
    assert min(expected_frontier(nbr, cnt, nodes, True)) >= 0


def test_hash_restatement_and_the_wrap_ids():
    # by hand: 1 * 0x9E3779B1 = 0x9E3779B1; >> 15 = 0x13C6E; low 16 bits 0x79B1 ^ 0x3C6E = 0x45DF
    assert hash_slot([1], 0xFFFF).tolist() == [0x45DF]
    assert hash_slot([0, 1, 1], 3).tolist() == [0, 3, 3]
    for count in (2, 8, 64, 1024):
        capacity = 4
        while capacity < 2 * count:
            capacity <<= 1                                          # ops.Frontier(max_ids=count): the highest load the host check admits
        ids = wrap_ids(capacity, count)
        assert ids.dtype == np.int32 and ids.size == count and np.unique(ids).size == count and ids.min() >= 0
        home = hash_slot(ids, capacity - 1)
        if count >= 4:
            assert (home == capacity - 1).sum() >= 2 and (home == capacity - 2).sum() >= 2
        else:
            assert (home == capacity - 1).sum() == 2                # two ids cannot do both: the second one wraps to slot 0
        # a sequential insert of these ids does wrap: some id ends below its home slot
        table, wrapped = {}, 0
        for x, h in zip(ids.tolist(), home.tolist()):
            s = h
            while s in table:
                s = (s + 1) & (capacity - 1)
            table[s] = x
            wrapped += s < h
        assert wrapped >= 1
