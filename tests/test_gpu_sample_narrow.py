"""GPU tests of the narrow sampler and the two-level hash frontier at their edge shapes (sage_sample_neighbors, sage_frontier_insert,
the one-launch sampler; csrc/sage_sample.hip, sage_sample_body.h, sage_hash_insert and sage_group_positions in sage_common.h; run with
-m gpu on an MI355X).

All of it is integer work and compared bit for bit.  The cases and the expected sets come from test_sample_narrow_host.py: graphs whose
degrees sit on every boundary of the kernel for each fanout of K_EDGE (both sides of every lane-group switch), node lists with repeats and
ids outside the graph, and test_sample_wide_host.wide_ref as the reference; that file also asserts, on the CPU, that the lists repeat ids
across blocks, inside blocks and among the nodes themselves.  A frontier's order is arbitrary, so it is compared as a set, with the slot
and row maps checked for consistency."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from sage355 import native, ops
from sage355.engine import TwoHopEngine
from sage355.graph import rmat_graph
from test_sample_narrow_host import K_EDGE, N_EDGE, SEED, edge_case, edge_ref, expected_frontier, lane_group, wrap_ids

pytestmark = pytest.mark.gpu
DEV = "cuda"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = -77
FIRST_ROW = 17
TAG = ops.TAG_OUTER            # the tag of every frontier test (the host file's conditions are stated for it)


def dev(a):
    return torch.tensor(np.asarray(a), device=DEV)


def device_case(k):
    rowptr, col, nodes = edge_case(k)
    return dev(rowptr), dev(col), dev(nodes)


def fresh_frontier(n, k, first_row=FIRST_ROW):
    return ops.Frontier(n * (k + 1), DEV, first_row=first_row)


def frontier_state(fr, first_row):
    """(total, ids of rows [first_row, total), keys, rows, nodes) on the host."""
    torch.cuda.synchronize()
    total = fr.size()
    listed = fr.nodes.cpu().numpy()
    return total, listed[first_row:total], fr.keys.cpu().numpy(), fr.rows.cpu().numpy(), listed


def check_frontier(fr, first_row, expect, nbr, cnt, slot, nodes=None, self_slot=None):
    """The frontier holds exactly `expect`, once each, in rows [first_row, total), and every slot handed out leads back to its id."""
    total, ids, keys, rows, listed = frontier_state(fr, first_row)
    assert (ids >= 0).all(), f"negative ids in the frontier: {ids[ids < 0].tolist()}"
    assert len(ids) == len(set(ids.tolist())), "frontier holds a duplicate"
    assert set(ids.tolist()) == expect                                                      # aggregators.py:52
    assert total - first_row == len(expect)
    k = nbr.shape[1]
    valid = np.arange(k)[None, :] < cnt[:, None]
    assert ((slot == -1) == ~valid).all()                                                   # -1 exactly on padding
    assert np.array_equal(keys[slot[valid]], nbr[valid])
    assert np.array_equal(listed[rows[slot[valid]]], nbr[valid])                            # aggregators.py:53,55
    if valid.any():
        assert rows[slot[valid]].min() >= first_row and rows[slot[valid]].max() < total
    filled = np.nonzero(keys != -1)[0]
    assert filled.size == len(expect) and np.array_equal(listed[rows[filled]], keys[filled])       # every key of the table has its row
    if self_slot is not None:
        inserted = nodes >= 0
        assert ((self_slot == -1) == ~inserted).all()                                       # a negative v is never inserted
        assert np.array_equal(keys[self_slot[inserted]], nodes[inserted])
        assert np.array_equal(listed[rows[self_slot[inserted]]], nodes[inserted])
    return total, ids


# ------------------------------------------------------------------------------------------------------------------------ a. the draw
@pytest.mark.parametrize("tag", [ops.TAG_INNER, ops.TAG_OUTER])
@pytest.mark.parametrize("k", K_EDGE)
def test_narrow_sampler_bit_exact_at_every_lane_group_boundary(k, tag):
    rowptr, col, nodes = device_case(k)
    nbr, cnt, slot, self_slot = ops.sample_neighbors(rowptr, col, nodes, k, seed=SEED, tag=tag)
    ref_nbr, ref_cnt = edge_ref(k, tag)
    assert slot is None and self_slot is None
    assert np.array_equal(cnt.cpu().numpy(), ref_cnt)
    assert np.array_equal(nbr.cpu().numpy(), ref_nbr)               # rows of ids outside the graph included: cnt 0, all -1
    outside = (edge_case(k)[2] < 0) | (edge_case(k)[2] >= rowptr.shape[0] - 1)
    assert outside.sum() == 4 and (ref_cnt[outside] == 0).all()


@pytest.mark.parametrize("k", K_EDGE)
def test_narrow_sampler_on_a_single_node(k):
    """n = 1: one lane group of one block, for the 70 000-neighbour node (Floyd's walk), a node taken whole and an id outside the graph."""
    rowptr, col, nodes = edge_case(k)
    deg = np.diff(rowptr)
    ref_nbr, ref_cnt = edge_ref(k, ops.TAG_INNER)
    rowptr_d, col_d = dev(rowptr), dev(col)
    for v in (int(np.argmax(deg)), int(np.nonzero(deg == k)[0][0]), -1):
        r = int(np.nonzero(nodes == v)[0][0])
        nbr, cnt, _, _ = ops.sample_neighbors(rowptr_d, col_d, dev(nodes[r:r + 1]), k, seed=SEED, tag=ops.TAG_INNER)
        assert int(cnt[0]) == ref_cnt[r] == (min(int(deg[v]), k) if v >= 0 else 0)
        assert np.array_equal(nbr.cpu().numpy()[0], ref_nbr[r])


# ---------------------------------------------------------------------------------------------------- b. the same draw with a frontier
@pytest.mark.parametrize("insert_self", [False, True])
@pytest.mark.parametrize("k", K_EDGE)
def test_narrow_frontier_is_the_set_union_with_consistent_maps(k, insert_self):
    rowptr, col, nodes = device_case(k)
    nodes_h = edge_case(k)[2]
    ref_nbr, ref_cnt = edge_ref(k, TAG)
    fr = fresh_frontier(N_EDGE, k)
    nbr, cnt, slot, self_slot = ops.sample_neighbors(rowptr, col, nodes, k, seed=SEED, tag=TAG, frontier=fr, insert_self=insert_self)
    assert np.array_equal(nbr.cpu().numpy(), ref_nbr) and np.array_equal(cnt.cpu().numpy(), ref_cnt)   # another instantiation, the same sets
    assert (self_slot is not None) == insert_self
    expect = expected_frontier(ref_nbr, ref_cnt, nodes_h, insert_self)
    total, ids = check_frontier(fr, FIRST_ROW, expect, ref_nbr, ref_cnt, slot.cpu().numpy(), nodes_h,
                                self_slot.cpu().numpy() if insert_self else None)
    # the wide entry on the same inputs and a fresh frontier: the same set, the same count, the same nodes inserted
    fw = fresh_frontier(N_EDGE, k)
    nbr_w, cnt_w, _, self_w = ops.sample_neighbors_wide(rowptr, col, nodes, k, seed=SEED, tag=TAG, frontier=fw, insert_self=insert_self)
    total_w, ids_w, _, _, _ = frontier_state(fw, FIRST_ROW)
    assert torch.equal(nbr_w, nbr) and torch.equal(cnt_w, cnt)
    assert total_w == total and set(ids_w.tolist()) == set(ids.tolist())
    if insert_self:
        assert torch.equal(self_w >= 0, self_slot >= 0)


# --------------------------------------------------------------------------------------------------------------- c. sage_frontier_insert
@pytest.mark.parametrize("with_self", [False, True])
@pytest.mark.parametrize("k", [8, 9, 33])
def test_frontier_insert_builds_the_same_frontier_from_given_lists(k, with_self):
    nodes_h = edge_case(k)[2]
    ref_nbr, ref_cnt = edge_ref(k, TAG)
    fr = fresh_frontier(N_EDGE, k)
    slot, self_slot = ops.frontier_insert(dev(ref_nbr), dev(ref_cnt), fr, self_nodes=dev(nodes_h) if with_self else None)
    assert (self_slot is not None) == with_self
    check_frontier(fr, FIRST_ROW, expected_frontier(ref_nbr, ref_cnt, nodes_h, with_self), ref_nbr, ref_cnt, slot.cpu().numpy(), nodes_h,
                   self_slot.cpu().numpy() if with_self else None)


# ------------------------------------------------------------------------------------------------------------------------ d. accumulation
@pytest.mark.parametrize("k", [8, 9, 33])
def test_a_second_call_adds_to_the_frontier_and_moves_no_row(k):
    """The two halves of the node list, one call each, into one frontier without a reset.  The list is put in the order of the node ids
    first (a node's draw does not depend on its place): as shuffled, every node is in both halves and the second call would add nothing."""
    rowptr, col, _ = device_case(k)
    order = np.argsort(edge_case(k)[2], kind="stable")
    nodes_h = edge_case(k)[2][order]
    nodes = dev(nodes_h)
    ref_nbr, ref_cnt = (a[order] for a in edge_ref(k, TAG))
    half = N_EDGE // 2
    fr = fresh_frontier(N_EDGE, k)
    _, _, slot_a, self_a = ops.sample_neighbors(rowptr, col, nodes[:half].contiguous(), k, seed=SEED, tag=TAG, frontier=fr, insert_self=True)
    expect_a = expected_frontier(ref_nbr[:half], ref_cnt[:half], nodes_h[:half], True)
    total_a, ids_a = check_frontier(fr, FIRST_ROW, expect_a, ref_nbr[:half], ref_cnt[:half], slot_a.cpu().numpy(), nodes_h[:half],
                                    self_a.cpu().numpy())
    rows_a = fr.rows.cpu().numpy().copy()
    _, _, slot_b, self_b = ops.sample_neighbors(rowptr, col, nodes[half:].contiguous(), k, seed=SEED, tag=TAG, frontier=fr, insert_self=True)
    expect = expected_frontier(ref_nbr, ref_cnt, nodes_h, True)     # = the one-call result (test b)
    assert expect > expect_a
    total, ids = check_frontier(fr, FIRST_ROW, expect, ref_nbr[half:], ref_cnt[half:], slot_b.cpu().numpy(), nodes_h[half:],
                                self_b.cpu().numpy())
    assert np.array_equal(ids[:total_a - FIRST_ROW], ids_a)         # every id of the first call keeps its row
    # an id the second call met again resolves to the row the first call gave it
    slot_b, rows = slot_b.cpu().numpy(), fr.rows.cpu().numpy()
    valid = np.arange(k)[None, :] < ref_cnt[half:, None]
    again = valid & np.isin(ref_nbr[half:], ids_a)
    assert again.sum() > 0 and (valid & ~again).sum() > 0
    assert (rows[slot_b[again]] < total_a).all() and np.array_equal(rows[slot_b[again]], rows_a[slot_b[again]])
    assert (rows[slot_b[valid & ~again]] >= total_a).all()


# ------------------------------------------------------------------------------------------------------------------------------ e. n_dev
@pytest.mark.parametrize("k", [8, 33])
def test_rows_past_the_device_count_are_not_written(k):
    """515 rows, 77 live: without a frontier (256-thread blocks) and with one (1024-thread blocks) whole blocks are inactive while they
    still run their barriers and their counter add."""
    rowptr, col, nodes = device_case(k)
    nodes_h = edge_case(k)[2]
    ref_nbr, ref_cnt = edge_ref(k, TAG)
    ref_nbr_d, ref_cnt_d = dev(ref_nbr), dev(ref_cnt)
    live = 77
    assert live % (256 // lane_group(k)) != 0 and live % (1024 // lane_group(k)) != 0
    n_dev = torch.tensor([live], dtype=torch.int32, device=DEV)
    expect_live = expected_frontier(ref_nbr[:live], ref_cnt[:live], nodes_h[:live], True)

    def buffers():
        return (torch.full((N_EDGE, k), SENTINEL, dtype=torch.int32, device=DEV), torch.full((N_EDGE,), SENTINEL, dtype=torch.int32, device=DEV))

    def check_rows(nbr, cnt, upto):
        assert bool((nbr[upto:] == SENTINEL).all()) and bool((cnt[upto:] == SENTINEL).all())
        assert torch.equal(nbr[:upto], ref_nbr_d[:upto]) and torch.equal(cnt[:upto], ref_cnt_d[:upto])

    # the narrow entry without a frontier
    nbr, cnt = buffers()
    ops.sample_neighbors(rowptr, col, nodes, k, seed=SEED, tag=TAG, n_dev=n_dev, out_nbr=nbr, out_cnt=cnt)
    check_rows(nbr, cnt, live)
    # with a frontier: the frontier of a 77-node call
    nbr, cnt = buffers()
    fr = fresh_frontier(N_EDGE, k)
    _, _, slot, self_slot = ops.sample_neighbors(rowptr, col, nodes, k, seed=SEED, tag=TAG, n_dev=n_dev, out_nbr=nbr, out_cnt=cnt, frontier=fr,
                                                 insert_self=True)
    check_rows(nbr, cnt, live)
    check_frontier(fr, FIRST_ROW, expect_live, ref_nbr[:live], ref_cnt[:live], slot.cpu().numpy()[:live], nodes_h[:live],
                   self_slot.cpu().numpy()[:live])
    # sage_frontier_insert
    fi = fresh_frontier(N_EDGE, k, first_row=0)
    slot, self_slot = ops.frontier_insert(ref_nbr_d, ref_cnt_d, fi, self_nodes=nodes, n_dev=n_dev)
    check_frontier(fi, 0, expect_live, ref_nbr[:live], ref_cnt[:live], slot.cpu().numpy()[:live], nodes_h[:live], self_slot.cpu().numpy()[:live])
    # a device count of 0 writes nothing
    n_dev.fill_(0)
    nbr, cnt = buffers()
    ops.sample_neighbors(rowptr, col, nodes, k, seed=SEED, tag=TAG, n_dev=n_dev, out_nbr=nbr, out_cnt=cnt)
    check_rows(nbr, cnt, 0)
    fr.reset(FIRST_ROW)
    ops.sample_neighbors(rowptr, col, nodes, k, seed=SEED, tag=TAG, n_dev=n_dev, out_nbr=nbr, out_cnt=cnt, frontier=fr, insert_self=True)
    check_rows(nbr, cnt, 0)
    fi.reset(0)
    ops.frontier_insert(ref_nbr_d, ref_cnt_d, fi, self_nodes=nodes, n_dev=n_dev)
    torch.cuda.synchronize()
    assert fr.size() == FIRST_ROW and fi.size() == 0 and bool((fr.keys == -1).all()) and bool((fi.keys == -1).all())
    # and one above n is capped at n
    n_dev.fill_(10_000)
    expect = expected_frontier(ref_nbr, ref_cnt, nodes_h, True)
    nbr, cnt = buffers()
    ops.sample_neighbors(rowptr, col, nodes, k, seed=SEED, tag=TAG, n_dev=n_dev, out_nbr=nbr, out_cnt=cnt)
    check_rows(nbr, cnt, N_EDGE)
    nbr, cnt = buffers()
    _, _, slot, self_slot = ops.sample_neighbors(rowptr, col, nodes, k, seed=SEED, tag=TAG, n_dev=n_dev, out_nbr=nbr, out_cnt=cnt, frontier=fr,
                                                 insert_self=True)
    check_rows(nbr, cnt, N_EDGE)
    check_frontier(fr, FIRST_ROW, expect, ref_nbr, ref_cnt, slot.cpu().numpy(), nodes_h, self_slot.cpu().numpy())
    slot, self_slot = ops.frontier_insert(ref_nbr_d, ref_cnt_d, fi, self_nodes=nodes, n_dev=n_dev)
    check_frontier(fi, 0, expect, ref_nbr, ref_cnt, slot.cpu().numpy(), nodes_h, self_slot.cpu().numpy())


# ----------------------------------------------------------------------------------------------------------------------- f. any_nonempty
@pytest.mark.parametrize("with_frontier", [False, True])
@pytest.mark.parametrize("k", [8, 64])
def test_any_nonempty_flag_of_the_narrow_entry(k, with_frontier):
    rowptr = torch.tensor([0, 0, 0, 0, 150, 150], dtype=torch.int64, device=DEV)   # node 3 has 150 neighbours, the others none
    col = torch.arange(150, dtype=torch.int32, device=DEV)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    per_block = (1024 if with_frontier else 256) // lane_group(k)
    n = 2 * per_block + 3                                                          # two full blocks and a partial one
    filler = np.resize(np.array([0, 1, 2, 4, 7], np.int32), n)                     # 7 is outside the graph: an empty row too
    kw = dict(seed=1, any_nonempty=flag)
    if with_frontier:
        kw.update(frontier=ops.Frontier(n * (k + 1), DEV), insert_self=True)
    _, cnt, _, _ = ops.sample_neighbors(rowptr, col, dev(filler), k, **kw)
    assert int(flag) == 0 and int(cnt.sum()) == 0
    mixed = filler.copy()
    mixed[-1] = 3                                                                  # the only neighboured node, in the last, partial block
    if with_frontier:
        kw["frontier"].reset(0)
    _, cnt, _, _ = ops.sample_neighbors(rowptr, col, dev(mixed), k, **kw)
    assert int(flag) == 1 and cnt.tolist() == [0] * (n - 1) + [k]


# -------------------------------------------------------------------------------------------------------------------- g. wrap and load
@pytest.mark.parametrize("n", [2, 8, 64, 1024])
def test_probing_wraps_past_the_last_slot_in_a_table_at_its_highest_load(n):
    fr = ops.Frontier(n, DEV)                                      # capacity = next_pow2(2 n): the smallest table the host check admits
    assert fr.capacity == ops.next_pow2(2 * n)
    ids = wrap_ids(fr.capacity, n)
    slot, _ = ops.frontier_insert(dev(ids[:, None].copy()), torch.ones(n, dtype=torch.int32, device=DEV), fr)
    check_frontier(fr, 0, set(ids.tolist()), ids[:, None], np.ones(n, np.int32), slot.cpu().numpy())
    fr.reset(0)
    torch.cuda.synchronize()
    assert fr.size() == 0 and bool((fr.keys == -1).all())


# ------------------------------------------------------------------------------------------------------------------ h. the max_nodes guard
class ShortFrontier:
    """A frontier whose nodes[] is declared shorter than the ids that will arrive, with a sentinel tail behind the declared end."""

    def __init__(self, capacity, max_nodes, tail=64):
        self.capacity, self.max_nodes = capacity, max_nodes
        self.keys = torch.empty(capacity, dtype=torch.int32, device=DEV)
        self.rows = torch.empty(capacity, dtype=torch.int32, device=DEV)
        self.nodes = torch.full((max_nodes + tail,), SENTINEL, dtype=torch.int32, device=DEV)
        self.count = torch.zeros(1, dtype=torch.int32, device=DEV)
        self.c = native.Frontier(self.keys.data_ptr(), self.rows.data_ptr(), capacity, self.nodes.data_ptr(), self.count.data_ptr(), max_nodes)
        native.check(native.lib().sage_frontier_reset(self.c, 0, native.stream_handle()), "frontier_reset")


@pytest.mark.parametrize("entry", ["sample", "insert"])
def test_ids_past_max_nodes_are_counted_but_not_listed(entry):
    k = 9
    rowptr, col, nodes = device_case(k)
    nodes_h = edge_case(k)[2]
    ref_nbr, ref_cnt = edge_ref(k, TAG)
    expect = expected_frontier(ref_nbr, ref_cnt, nodes_h, True)
    max_nodes = len(expect) // 2
    fr = ShortFrontier(ops.next_pow2(2 * N_EDGE * (k + 1)), max_nodes)
    if entry == "sample":
        ops.sample_neighbors(rowptr, col, nodes, k, seed=SEED, tag=TAG, frontier=fr, insert_self=True)
    else:
        ops.frontier_insert(dev(ref_nbr), dev(ref_cnt), fr, self_nodes=nodes)
    torch.cuda.synchronize()
    listed = fr.nodes.cpu().numpy()
    assert (listed[max_nodes:] == SENTINEL).all()                    # nothing behind the declared end
    assert int(fr.count) == len(expect)                              # the counter still says how many there were
    head = listed[:max_nodes]
    assert len(set(head.tolist())) == max_nodes and set(head.tolist()) <= expect


# ------------------------------------------------------------------------------------------------------- i. the engine with bad device ids
@pytest.fixture(scope="module")
def small_problem():
    graph = rmat_graph(12, 40_000, seed=2, accel=None)
    gen = torch.Generator().manual_seed(0)
    d0, h1, h2 = 64, 32, 16
    table = torch.randn(graph.num_nodes, d0, generator=gen)
    w1 = {m: torch.randn(h1, m * d0, generator=gen) / np.sqrt(m * d0) for m in (1, 2)}
    w2 = {m: torch.randn(h2, m * h1, generator=gen) / np.sqrt(m * h1) for m in (1, 2)}
    return graph, table, w1, w2


@pytest.mark.parametrize("relabel", [None, "degree"])
@pytest.mark.parametrize("concat,self_loop", [(False, True), (True, False), (True, True)])
def test_engine_keeps_bad_device_ids_out_of_the_frontier(small_problem, concat, self_loop, relabel):
    """Device-resident seeds outside [0, num_nodes) are isolated nodes (the reference raises for them): they sample nothing, a negative
    one -- which is what every bad seed becomes behind the degree layout's seed map -- adds no row to the frontier, and the good seeds'
    outputs are what they are without the bad ones."""
    graph, table, w1, w2 = small_problem
    m = 2 if concat else 1
    rp, cl = graph.to(DEV)

    def engine():
        return TwoHopEngine(rp, cl, table.to(DEV), w1[m].to(DEV), w2[m].to(DEV), 5, 5, max_batch=9, nan_empty=False, concat=concat,
                            agg_self_loop=self_loop, relabel=relabel)

    good = np.nonzero(graph.degrees() > 0)[0][:6].astype(np.int32)
    ids = dev(np.concatenate([good, np.array([graph.num_nodes + 5, -3, -1], np.int32)]))
    eng = engine()
    out = eng.forward(ids, seed=1).clone()
    it = eng.intermediates()
    cnt2 = it["cnt2"].cpu().numpy()
    assert (cnt2[:6] > 0).all() and (cnt2[6:] == 0).all()
    first = it["first_frontier_row"]
    s1 = it["s1_nodes"].cpu().numpy()[first:]
    assert (s1 >= 0).all(), f"negative ids in the frontier: {s1[s1 < 0].tolist()}"
    if relabel:
        s1 = eng.node_order.cpu().numpy()[s1]                       # back to the caller's ids
    assert len(set(s1.tolist())) == len(s1), "frontier holds a duplicate"
    assert it["n_s1"] - first == len(set(s1.tolist()))
    alone = engine().forward(dev(good), seed=1)
    assert torch.equal(out[:6], alone)


# ------------------------------------------------------------------------------------------ j. the one-launch sampler's lane-group pairs
FUSED_SCRIPT = r"""
import sys
sys.path[:0] = [{repo!r}, {repo!r} + "/graphsage-simple_amd", {repo!r} + "/tests"]
import numpy as np, torch
from sage355.graph import rmat_graph
from test_gpu_forward import check_engine_against_oracle
graph = rmat_graph(12, 60_000)
gen = torch.Generator().manual_seed(0)
seeds = np.random.default_rng(1).choice(np.nonzero(graph.degrees() > 0)[0], 300, replace=False)
table = torch.randn(graph.num_nodes, 128, generator=gen)
pairs = [(k2, k1) for k2 in (16, 17, 33) for k1 in (16, 17, 33)] + [(1, 64), (64, 1)]
for concat, self_loop in ((False, True), (True, False)):
    m = 2 if concat else 1
    w1 = torch.randn(128, m * 128, generator=gen) / np.sqrt(m * 128)
    w2 = torch.randn(64, m * 128, generator=gen) / np.sqrt(m * 128)
    for k2, k1 in pairs:
        err = check_engine_against_oracle(graph, table, w1, w2, seeds, k1, k2, concat, self_loop, True)
        print("ok", k2, k1, concat, self_loop, err)
print("FUSED_SAMPLER_OK")
"""


@pytest.mark.parametrize("threads", ["512", "1024"])
def test_one_launch_sampler_at_every_lane_group_pair(threads, tmp_path):
    """SAGE_SAMPLE_FUSED=1 (both hops in one launch) has 3 x 3 (outer, inner) lane-group pairs times two block sizes: every pair, with
    fanouts on both sides of the switches, against the C sampler bit for bit and the fp64 oracle, in one child process per block size
    (the tunables are read once per process).  The widths are those of test_fused_sampler_leaves_the_same_sets_and_rows, where layer 2
    is a one-launch layer, the condition for this sampler; the engine does not report which sampler ran."""
    script = tmp_path / "fused_pairs.py"
    script.write_text(FUSED_SCRIPT.format(repo=REPO))
    e = dict(os.environ)
    e.update(SAGE_SAMPLE_FUSED="1", SAGE_SO_THREADS=threads)
    res = subprocess.run([sys.executable, str(script)], env=e, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and "FUSED_SAMPLER_OK" in res.stdout, res.stdout[-2000:] + res.stderr[-3000:]
    assert len([line for line in res.stdout.splitlines() if line.startswith("ok ")]) == 2 * 11
