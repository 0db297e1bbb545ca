"""GPU tests of the wide sampler (sage_sample_neighbors_wide, fanouts up to 1024; run with -m gpu on an MI355X).

All of it is integer work and compared bit for bit.  The expected sets above k = 64 come from test_sample_wide_host.wide_ref, the Python
restatement of oracle/sampler_ref.c's rule (that file stops at 64); at k <= 64 the wide entry must equal both the narrow entry and the C
oracle.  The statistical test asks for the reference's distribution (aggregators.py:42-46: a uniform k-subset) within 6-sigma bands."""
import numpy as np
import pytest
import torch

from oracle import sampler_ref
from sage355 import native, ops
from sage355.graph import rmat_graph
from test_sample_wide_host import wide_ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
SEED = 0xC0FFEE1234
SENTINEL = -77


@pytest.fixture(scope="module")
def graph():
    g = rmat_graph(13, 200_000, seed=3)
    return g, torch.from_numpy(g.rowptr).to(DEV), torch.from_numpy(g.col).to(DEV)


def edge_csr(k):
    """A CSR whose degrees sit on every boundary of the kernel for fanout k (take-all / Floyd, the 64-slot chunks), some random ones
    between, and 203 node ids in shuffled order, two of them outside [0, num_nodes)."""
    rng = np.random.default_rng(k)
    deg = np.array([0, 1, 63, 64, 65, k - 1, k, k + 1, 2 * k + 3, 5000] + rng.integers(0, 3 * k, 30).tolist(), dtype=np.int64)
    deg = deg[rng.permutation(deg.size)]
    num_nodes = deg.size
    rowptr = np.zeros(num_nodes + 1, np.int64)
    rowptr[1:] = np.cumsum(deg)
    col = rng.integers(0, 1 << 30, int(rowptr[-1])).astype(np.int32)      # ids are opaque to the sampler: it reports col[] entries
    nodes = np.concatenate([rng.permutation(num_nodes), rng.integers(0, num_nodes, 201 - num_nodes), [num_nodes, -5]]).astype(np.int32)
    nodes = nodes[rng.permutation(nodes.size)]
    assert nodes.size == 203
    return rowptr, col, nodes


@pytest.mark.parametrize("tag", [ops.TAG_INNER, ops.TAG_OUTER])
@pytest.mark.parametrize("k", [65, 100, 128, 129, 256, 1000, 1024])
def test_wide_sampler_bit_exact_vs_the_restatement(k, tag):
    rowptr, col, nodes = edge_csr(k)
    nbr, cnt, _, _ = ops.sample_neighbors_wide(torch.from_numpy(rowptr).to(DEV), torch.from_numpy(col).to(DEV),
                                               torch.from_numpy(nodes).to(DEV), k, seed=SEED, tag=tag)
    ref_nbr, ref_cnt = wide_ref(rowptr, col, nodes, k, SEED, tag)
    assert np.array_equal(cnt.cpu().numpy(), ref_cnt)
    assert np.array_equal(nbr.cpu().numpy(), ref_nbr)


@pytest.mark.parametrize("k", [1, 25, 64])
def test_wide_equals_narrow_and_the_c_oracle_at_narrow_fanouts(graph, k):
    g, rowptr, col = graph
    rs = np.random.default_rng(k)
    nodes = rs.integers(0, g.num_nodes, size=5000).astype(np.int32)
    nodes[:50] = np.argsort(-g.degrees())[:50]          # the hubs
    nodes_d = torch.from_numpy(nodes).to(DEV)
    nbr, cnt, _, _ = ops.sample_neighbors_wide(rowptr, col, nodes_d, k, seed=SEED, tag=ops.TAG_INNER)
    nbr_n, cnt_n, _, _ = ops.sample_neighbors(rowptr, col, nodes_d, k, seed=SEED, tag=ops.TAG_INNER)
    ref_nbr, ref_cnt = sampler_ref.sample_neighbors(g.rowptr, g.col, nodes, k, SEED, ops.TAG_INNER)
    assert torch.equal(cnt, cnt_n) and torch.equal(nbr, nbr_n)
    assert np.array_equal(cnt.cpu().numpy(), ref_cnt) and np.array_equal(nbr.cpu().numpy(), ref_nbr)


def test_rows_past_the_device_count_are_not_written():
    k = 100
    rowptr, col, nodes = edge_csr(k)
    rowptr_d, col_d, nodes_d = torch.from_numpy(rowptr).to(DEV), torch.from_numpy(col).to(DEV), torch.from_numpy(nodes).to(DEV)
    full_nbr, full_cnt, _, _ = ops.sample_neighbors_wide(rowptr_d, col_d, nodes_d, k, seed=SEED, tag=ops.TAG_INNER)
    n_dev = torch.tensor([77], dtype=torch.int32, device=DEV)
    nbr = torch.full((203, k), SENTINEL, dtype=torch.int32, device=DEV)
    cnt = torch.full((203,), SENTINEL, dtype=torch.int32, device=DEV)
    ops.sample_neighbors_wide(rowptr_d, col_d, nodes_d, k, seed=SEED, tag=ops.TAG_INNER, n_dev=n_dev, out_nbr=nbr, out_cnt=cnt)
    assert bool((nbr[77:] == SENTINEL).all()) and bool((cnt[77:] == SENTINEL).all())
    assert torch.equal(nbr[:77], full_nbr[:77]) and torch.equal(cnt[:77], full_cnt[:77])
    # a device count above n is capped at n
    n_dev.fill_(1000)
    ops.sample_neighbors_wide(rowptr_d, col_d, nodes_d, k, seed=SEED, tag=ops.TAG_INNER, n_dev=n_dev, out_nbr=nbr, out_cnt=cnt)
    assert torch.equal(nbr, full_nbr) and torch.equal(cnt, full_cnt)


def test_draw_depends_only_on_seed_tag_and_node():
    k = 100
    rowptr, col, nodes = edge_csr(k)
    rowptr_d, col_d, nodes_d = torch.from_numpy(rowptr).to(DEV), torch.from_numpy(col).to(DEV), torch.from_numpy(nodes).to(DEV)
    nbr, cnt, _, _ = ops.sample_neighbors_wide(rowptr_d, col_d, nodes_d, k, seed=SEED, tag=ops.TAG_INNER)
    perm = torch.from_numpy(np.random.default_rng(1).permutation(203)).to(DEV)
    nbr_p, cnt_p, _, _ = ops.sample_neighbors_wide(rowptr_d, col_d, nodes_d[perm].contiguous(), k, seed=SEED, tag=ops.TAG_INNER)
    assert torch.equal(nbr_p, nbr[perm]) and torch.equal(cnt_p, cnt[perm])
    r = int(np.nonzero(nodes == np.argmax(np.diff(rowptr)))[0][0])                  # a row of the 5000-neighbour node
    assert int(cnt[r]) == k
    nbr_1, cnt_1, _, _ = ops.sample_neighbors_wide(rowptr_d, col_d, nodes_d[r:r + 1].contiguous(), k, seed=SEED, tag=ops.TAG_INNER)
    assert torch.equal(nbr_1[0], nbr[r]) and int(cnt_1[0]) == k
    nbr_t, cnt_t, _, _ = ops.sample_neighbors_wide(rowptr_d, col_d, nodes_d, k, seed=SEED, tag=ops.TAG_OUTER)
    floyd = cnt == k
    assert torch.equal(cnt_t, cnt) and not torch.equal(nbr_t[floyd], nbr[floyd])
    assert not torch.equal(nbr_t[r], nbr[r])


def test_contract_distinct_members_takeall(graph):
    """aggregators.py:42-46: deg >= k -> k distinct neighbours; deg < k -> all of them."""
    g, rowptr, col = graph
    k = 100
    nodes = np.arange(g.num_nodes, dtype=np.int32)
    nbr, cnt, _, _ = ops.sample_neighbors_wide(rowptr, col, torch.from_numpy(nodes).to(DEV), k, seed=7, tag=ops.TAG_OUTER)
    nbr, cnt = nbr.cpu().numpy(), cnt.cpu().numpy()
    deg = g.degrees()
    assert (deg > k).sum() > 50 and (deg <= k).sum() > 50
    assert np.array_equal(cnt, np.minimum(deg, k))
    assert ((np.arange(k)[None, :] >= cnt[:, None]) == (nbr == -1)).all()          # padding is -1, and only padding
    for v in range(g.num_nodes):
        row = nbr[v, :cnt[v]]
        if deg[v] <= k:
            assert np.array_equal(row, g.neighbors(v))                              # CSR order
        else:
            members = set(g.neighbors(v).tolist())
            assert len(set(row.tolist())) == k and set(row.tolist()) <= members


@pytest.mark.parametrize("deg,k,trials", [(200, 80, 20000), (300, 129, 20000), (2000, 1024, 4000)])
def test_wide_sampler_is_uniform_without_replacement(deg, k, trials):
    """`trials` nodes that all have the same `deg` neighbours: every neighbour must be chosen with probability k / deg and every unordered
    pair with k (k-1) / (deg (deg-1)), within 6-sigma bands (the Python restatement alone sits at 3.2 .. 4.8 sigma on these inputs)."""
    rowptr = torch.arange(trials + deg + 1, dtype=torch.int64).clamp(max=trials) * deg
    col = (trials + torch.arange(deg, dtype=torch.int32)).repeat(trials)
    nodes = torch.arange(trials, dtype=torch.int32)
    nbr, cnt, _, _ = ops.sample_neighbors_wide(rowptr.to(DEV), col.to(DEV), nodes.to(DEV), k, seed=2718281828, tag=5)
    rows = nbr.cpu().numpy().astype(np.int64) - trials
    assert (cnt.cpu().numpy() == k).all() and rows.min() >= 0 and rows.max() < deg
    member = np.zeros((trials, deg), dtype=np.float32)
    member[np.arange(trials)[:, None], rows] = 1.0
    assert (member.sum(1) == k).all()                                               # distinct
    hits = member.sum(0, dtype=np.float64)
    p = k / deg
    z1 = np.abs(hits - trials * p).max() / np.sqrt(trials * p * (1 - p))
    pair = torch.from_numpy(member).t() @ torch.from_numpy(member)     # co-occurrence counts: integers <= trials, exact in fp32
    pp = k * (k - 1) / (deg * (deg - 1))
    off = pair.numpy().astype(np.float64)[~np.eye(deg, dtype=bool)]
    z2 = np.abs(off - trials * pp).max() / np.sqrt(trials * pp * (1 - pp))
    print(f"deg={deg} k={k} trials={trials}: max z single = {z1:.2f}, pair = {z2:.2f}")
    assert z1 < 6, z1
    assert z2 < 6, z2


@pytest.mark.parametrize("insert_self", [False, True])
def test_wide_frontier_is_the_set_union_with_a_consistent_row_map(graph, insert_self):
    g, rowptr, col = graph
    k = 100
    rs = np.random.default_rng(11)
    deg = g.degrees()
    nodes = rs.choice(np.nonzero(deg > 0)[0], 1500, replace=False).astype(np.int32)
    nodes_d = torch.from_numpy(nodes).to(DEV)
    first_row = 17
    fr = ops.Frontier(nodes.size * (k + 1), DEV, first_row=first_row)
    nbr, cnt, slot, self_slot = ops.sample_neighbors_wide(rowptr, col, nodes_d, k, seed=99, tag=ops.TAG_OUTER, frontier=fr,
                                                          insert_self=insert_self)
    torch.cuda.synchronize()
    total = fr.size()
    ids = fr.nodes[first_row:total].cpu().numpy()
    nbr_h, cnt_h, slot_h = nbr.cpu().numpy(), cnt.cpu().numpy(), slot.cpu().numpy()
    ref_nbr, ref_cnt = wide_ref(g.rowptr, g.col, nodes, k, 99, ops.TAG_OUTER)
    assert np.array_equal(nbr_h, ref_nbr) and np.array_equal(cnt_h, ref_cnt)      # the frontier variant draws the same sets
    valid = np.arange(k)[None, :] < cnt_h[:, None]
    expect = set(nbr_h[valid].tolist()) | (set(nodes.tolist()) if insert_self else set())
    assert len(ids) == len(set(ids.tolist())), "frontier holds a duplicate"
    assert set(ids.tolist()) == expect                                    # aggregators.py:52
    assert total - first_row == len(expect)
    rows = fr.rows.cpu().numpy()
    keys = fr.keys.cpu().numpy()
    listed = fr.nodes.cpu().numpy()
    assert (slot_h[~valid] == -1).all()
    assert np.array_equal(keys[slot_h[valid]], nbr_h[valid])
    assert np.array_equal(listed[rows[slot_h[valid]]], nbr_h[valid])        # aggregators.py:53,55
    assert rows[slot_h[valid]].min() >= first_row and rows[slot_h[valid]].max() < total
    if insert_self:
        ss = self_slot.cpu().numpy()
        assert np.array_equal(keys[ss], nodes) and np.array_equal(listed[rows[ss]], nodes)
    else:
        assert self_slot is None


def test_any_nonempty_flag():
    rowptr = torch.tensor([0, 0, 0, 0, 150, 150], dtype=torch.int64, device=DEV)   # node 3 has 150 neighbours, the others none
    col = torch.arange(150, dtype=torch.int32, device=DEV)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    isolated = torch.tensor([0, 1, 2, 4, 0, 1, 2, 4, 7], dtype=torch.int32, device=DEV)    # 7 is outside the graph: an empty row too
    _, cnt, _, _ = ops.sample_neighbors_wide(rowptr, col, isolated, 100, seed=1, any_nonempty=flag)
    assert int(flag) == 0 and int(cnt.sum()) == 0
    mixed = torch.tensor([0, 1, 2, 4, 0, 1, 3], dtype=torch.int32, device=DEV)
    _, cnt, _, _ = ops.sample_neighbors_wide(rowptr, col, mixed, 100, seed=1, any_nonempty=flag)
    assert int(flag) == 1 and cnt.tolist() == [0, 0, 0, 0, 0, 0, 100]


def test_the_picking_wrapper_and_the_limits():
    rowptr = torch.tensor([0, 150], dtype=torch.int64, device=DEV)
    col = torch.arange(150, dtype=torch.int32, device=DEV)
    nodes = torch.zeros(3, dtype=torch.int32, device=DEV)
    for k in (64, 65):
        a = ops.sample_neighbors_any(rowptr, col, nodes, k, seed=3)
        b = ops.sample_neighbors_wide(rowptr, col, nodes, k, seed=3)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    with pytest.raises(native.SageError):
        ops.sample_neighbors(rowptr, col, nodes, 65, seed=3)                   # the narrow entry keeps its limit
    with pytest.raises(native.SageError):
        ops.sample_neighbors_any(rowptr, col, nodes, native.MAX_FANOUT_WIDE + 1, seed=3)    # refused on the host
