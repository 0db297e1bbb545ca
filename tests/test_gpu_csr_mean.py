"""sage_csr_mean (full-neighbourhood mean straight from the CSR, aggregators.py:47-48 num_sample=None) on the MI355X:
against fp64 row sums computed by torch on the CPU, the reference's NaN / zero rule, and bitwise reproducibility."""
import numpy as np
import pytest
import torch

from sage355 import native, ops
from sage355.graph import rmat_graph
from sage355.inference import _nonempty_flag
from util import assert_close_rowmax, csr_row_sums, csr_rows_reference, load_golden, plan_gamma, plan_miss

pytestmark = pytest.mark.gpu


def bits_equal(a, b):
    """Bitwise equality, NaNs included (torch.equal says NaN != NaN)."""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))
E = native.CSR_MEAN_CHUNK


def skewed_graph(seed=0):
    """Rows of degree 0, 1, E-1, E, E+1, 2E, 2E+1 and one star hub of 20E + 37, among rows of 0..6 edges; some rows hold
    their own node (a self-loop edge), neighbour lists unsorted."""
    rng = np.random.default_rng(seed)
    n = 24 * E
    special = {0: 0, 1: 1, 2: E - 1, 3: E, 4: E + 1, 5: 2 * E, 6: 2 * E + 1, 7: 20 * E + 37, 8: E + 1, 9: 2 * E + 1}
    deg = rng.integers(0, 7, n)
    for v, d in special.items():
        deg[v] = d
    rowptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(deg, out=rowptr[1:])
    col = rng.integers(0, n, int(rowptr[-1])).astype(np.int32)
    col[rowptr[7]:rowptr[8]] = rng.permutation(n)[: deg[7]]          # the hub: a star over distinct nodes
    for v in (3, 8, 9, 20, 21, 22):                                     # self-loop edges (rows 8, 9 in their last chunk)
        if deg[v] > 0:
            col[rowptr[v + 1] - 1] = v
    col[rowptr[7] + 5 * E + 3] = 7
    return rowptr, col


def fp64_mean(rowptr, col, table64, nodes, self_loop, nan_flag):
    """[len(nodes), dim] float64: sum over the CSR row (plus the node itself when self_loop and absent), / count."""
    out = torch.zeros(len(nodes), table64.shape[1], dtype=torch.float64)
    for r, v in enumerate(nodes):
        ids = col[rowptr[v]:rowptr[v + 1]]
        s = table64[torch.from_numpy(ids.astype(np.int64))].sum(0)
        c = len(ids)
        if self_loop and not np.any(ids == v):
            s = s + table64[v]
            c += 1
        out[r] = s / c if c else (float("nan") if nan_flag else 0.0)
    return out


@pytest.fixture(scope="module")
def graph():
    rowptr, col = skewed_graph()
    return rowptr, col, torch.from_numpy(rowptr).cuda(), torch.from_numpy(col).cuda()


@pytest.mark.parametrize("dim,pad", [(1, 0), (3, 0), (4, 0), (50, 3), (256, 0), (256, 4), (1433, 0)])
def test_csr_mean_against_fp64_row_sums(graph, dim, pad):
    rowptr, col, rp, cl = graph
    n = rowptr.shape[0] - 1
    gen = torch.Generator().manual_seed(dim)
    wide = torch.randn(n, dim + pad, generator=gen)
    table = wide.cuda()[:, :dim] if pad else wide.cuda()             # pad > 0: ld > dim
    table64 = wide[:, :dim].double()
    rng = np.random.default_rng(dim)
    subset = np.concatenate([np.arange(10), [7, 7, 5, 0], rng.integers(0, n, 200), [21, 9]]).astype(np.int64)
    flag = torch.ones(1, dtype=torch.int32, device="cuda")
    sums = csr_row_sums(rowptr, col, wide[:, :dim].numpy())
    for self_loop in (False, True):
        full = ops.csr_mean(rp, cl, table, self_loop=self_loop, any_nonempty=flag)
        exp_rows = np.concatenate([np.arange(40), [7, 8, 9]])
        assert_close_rowmax(full.cpu()[exp_rows], fp64_mean(rowptr, col, table64, exp_rows, self_loop, True),
                            what=f"all rows dim={dim} ld={dim + pad} self_loop={self_loop}")
        ref, bar, _ = csr_rows_reference(rowptr, col, wide[:, :dim].numpy(), self_loop=self_loop, flag=True, sums=sums)
        miss = plan_miss(full.cpu().numpy(), ref, bar, f"every row, per element: dim={dim} ld={dim + pad} self_loop={self_loop}")
        assert miss is None, miss
        sub = ops.csr_mean(rp, cl, table, nodes=torch.from_numpy(subset.astype(np.int32)).cuda(), self_loop=self_loop, any_nonempty=flag)
        assert_close_rowmax(sub.cpu(), fp64_mean(rowptr, col, table64, subset, self_loop, True),
                            what=f"subset dim={dim} self_loop={self_loop}")
        assert bits_equal(sub.cpu(), full.cpu()[torch.from_numpy(subset)]), "csr_mean(nodes=S) != csr_mean()[S] bitwise"


def test_csr_mean_workspace_bound_costs_speed_not_bits(graph):
    """A max_edges below the truth leaves long rows without workspace room: their row wave sums the chunks itself, in the same
    order.  The result is the same bits, with no room at all (max_edges = 0) and with room for some of the chunks."""
    rowptr, col, rp, cl = graph
    table = torch.randn(rowptr.shape[0] - 1, 64, generator=torch.Generator().manual_seed(5)).cuda()
    ref = ops.csr_mean(rp, cl, table, self_loop=True)
    for max_edges in (0, 3 * E, 25 * E):
        assert bits_equal(ops.csr_mean(rp, cl, table, self_loop=True, max_edges=max_edges), ref), max_edges


def test_csr_mean_rejects_a_short_workspace(graph):
    _, _, rp, cl = graph
    table = torch.zeros(rp.shape[0] - 1, 8, device="cuda")
    need = ops.csr_mean_workspace_bytes(rp.shape[0] - 1, cl.numel(), 8)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    out = torch.empty(rp.shape[0] - 1, 8, device="cuda")
    rc = native.lib().sage_csr_mean(native.ptr(rp), native.ptr(cl), rp.shape[0] - 1, None, rp.shape[0] - 1, cl.numel(),
                                    native.ptr(table), table.shape[0], 8, 8, 0, None, native.ptr(out), 8, native.ptr(ws), need - 256,
                                    native.stream_handle())
    assert rc == native.ENOSPACE and b"workspace" in native.lib().sage_last_error()


def test_csr_mean_nan_and_zero_rule():
    """tests/golden/empty_sets.npz: an empty set in a batch with edges is the reference's 0/0 = NaN, an all-empty batch zeros."""
    g = load_golden("empty_sets")
    table = torch.from_numpy(g["table"]).cuda()
    n = table.shape[0]
    sets = {int(v): g["nbr"][r, :int(g["cnt"][r])] for r, v in enumerate(g["nodes"])}
    deg = np.zeros(n, dtype=np.int64)
    for v, s in sets.items():
        deg[v] = len(s)
    rowptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(deg, out=rowptr[1:])
    col = np.concatenate([sets.get(v, np.zeros(0, np.int64)) for v in range(n)]).astype(np.int32)
    rp, cl = torch.from_numpy(rowptr).cuda(), torch.from_numpy(col).cuda()
    nodes = torch.from_numpy(g["nodes"].astype(np.int32)).cuda()
    mixed = ops.csr_mean(rp, cl, table, nodes=nodes, any_nonempty=_nonempty_flag(rp))
    assert_close_rowmax(mixed.cpu(), g["agg_mixed"], what="agg_mixed")
    empty_rp = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    empty_cl = torch.zeros(0, dtype=torch.int32, device="cuda")
    both_empty = torch.tensor([3, 5], dtype=torch.int32, device="cuda")
    allempty = ops.csr_mean(empty_rp, empty_cl, table, nodes=both_empty, any_nonempty=_nonempty_flag(empty_rp))
    assert_close_rowmax(allempty.cpu(), g["agg_all_empty"], what="agg_all_empty")
    assert torch.equal(ops.csr_mean(rp, cl, table, nodes=nodes).isnan().cpu(), torch.zeros(4, table.shape[1], dtype=torch.bool))


def test_csr_mean_reproducible_on_rmat():
    g = rmat_graph(16, 1_000_000, seed=3)
    deg = g.degrees()
    assert int(deg.max()) > 16 * E and int((deg > E).sum()) > 100     # max degree 9,423; 697 rows over 512
    rp, cl = g.to("cuda")
    table = torch.randn(g.num_nodes, 256, generator=torch.Generator().manual_seed(3)).cuda()
    flag = _nonempty_flag(rp)
    a = ops.csr_mean(rp, cl, table, self_loop=True, any_nonempty=flag)
    b = ops.csr_mean(rp, cl, table, self_loop=True, any_nonempty=flag)
    assert bits_equal(a, b), "two calls differ"
    rng = np.random.default_rng(3)
    hubs = np.argsort(deg)[-64:]
    s = np.concatenate([hubs, rng.integers(0, g.num_nodes, 4000), hubs[::-1]]).astype(np.int32)
    sub = ops.csr_mean(rp, cl, table, nodes=torch.from_numpy(s).cuda(), self_loop=True, any_nonempty=flag)
    assert bits_equal(sub, a[torch.from_numpy(s.astype(np.int64)).cuda()]), "csr_mean(nodes=S) != csr_mean()[S] bitwise"
    hub = int(np.argmax(deg))
    ids = torch.from_numpy(g.neighbors(hub).astype(np.int64))
    t64 = table.cpu().double()
    own = hub in set(g.neighbors(hub).tolist())
    expect = (t64[ids].sum(0) + (0 if own else t64[hub])) / (len(ids) + (0 if own else 1))
    assert_close_rowmax(a[hub:hub + 1].cpu(), expect[None], what="max-degree row")


# ------------------------------------------------------------------------------------------------------------------------------
# The written contract of sage_csr_mean (include/sage355.h, csrc/sage_csr_common.h: row_span, sum_edges): what is not written, and
# what out-of-range node ids, neighbour ids and row pointers do.  Every call is safe even if a clamp were missing -- the table, col
# and rowptr are the MIDDLE of larger allocations with G guard rows / entries on either side and no value is out of range by more
# than G -- so that a missing clamp shows as wrong numbers (the guard rows hold 1e30), never as an access outside an allocation.
G = 8
SENTINEL_BITS = 0x7FC0BEEF                       # a NaN with a payload: neither a result nor the kernel's own NaN (0x7FC00000)


class Guarded:
    """A CSR and a table as device views into guarded allocations.  rowptr int64 [num_nodes + 1] (guards: 0 before, the total
    behind), col int32 [E] (guards: ids of guard rows), table [table_rows, dim] with leading dimension ld (guards: 1e30)."""

    def __init__(self, rowptr, col, table, ld=None):
        rowptr, col = np.asarray(rowptr, dtype=np.int64), np.asarray(col, dtype=np.int32)
        self.num_nodes, self.edges = len(rowptr) - 1, len(col)
        self.table_rows, self.dim = table.shape
        self.ld = self.dim if ld is None else ld
        rp = np.concatenate([np.zeros(G, np.int64), rowptr, np.full(G, max(int(rowptr[-1]), 0), np.int64)])
        cl = np.concatenate([-1 - np.arange(G, dtype=np.int32), col, self.table_rows + np.arange(G, dtype=np.int32)])
        tb = np.full((self.table_rows + 2 * G, self.ld), 1e30, dtype=np.float32)
        tb[G:G + self.table_rows, :self.dim] = table
        self._keep = (torch.from_numpy(rp).cuda(), torch.from_numpy(cl).cuda(), torch.from_numpy(tb).cuda())
        self.rp = self._keep[0][G:G + self.num_nodes + 1]
        self.cl = self._keep[1][G:G + max(self.edges, 1)]
        self.table = self._keep[2][G:G + self.table_rows, :self.dim]

    def mean(self, nodes=None, self_loop=False, flag=None, max_edges=None, table_rows=None):
        """sage_csr_mean through the C entry (the wrapper insists on table_rows >= num_nodes) -> out [n, dim]"""
        n = self.num_nodes if nodes is None else nodes.shape[0]
        me = self.edges if max_edges is None else max_edges
        out = torch.full((n, self.dim), 7.0, device="cuda")
        need = ops.csr_mean_workspace_bytes(n, me, self.dim)
        ws = torch.full((need + 256,), 0xA5, dtype=torch.uint8, device="cuda")
        P = native.ptr
        rc = native.lib().sage_csr_mean(P(self.rp), P(self.cl), self.num_nodes, P(nodes), n, me, P(self.table),
                                        self.table_rows if table_rows is None else table_rows, self.ld, self.dim, 1 if self_loop else 0, P(flag),
                                        P(out), self.dim, P(ws), need, native.stream_handle())
        native.check(rc, "csr_mean")
        assert bool((ws[need:] == 0xA5).all()), "csr_mean wrote past its workspace"
        return out


def _flag(value):
    return torch.full((1,), value, dtype=torch.int32, device="cuda")


def _small_csr(num_nodes, long_row, seed, long_deg=2 * E + 1):
    """Rows of 0..6 entries over ids in [0, num_nodes), row `long_row` with long_deg, rows 0 and num_nodes - 1 empty."""
    rng = np.random.default_rng(seed)
    deg = rng.integers(0, 7, num_nodes)
    deg[long_row] = long_deg
    deg[0] = deg[num_nodes - 1] = 0
    rowptr = np.zeros(num_nodes + 1, dtype=np.int64)
    np.cumsum(deg, out=rowptr[1:])
    return rowptr, rng.integers(0, num_nodes, int(rowptr[-1])).astype(np.int32)


@pytest.mark.parametrize("dim,pad", [(3, 2), (4, 4), (50, 3), (256, 4)])
def test_csr_mean_writes_every_row_of_out_and_nothing_else(graph, dim, pad):
    rowptr, col, rp, cl = graph
    n = rowptr.shape[0] - 1
    table = torch.randn(n, dim, generator=torch.Generator().manual_seed(dim)).cuda()
    flag = _flag(1)
    for nodes in (None, torch.arange(n - 40, -1, -1, dtype=torch.int32, device="cuda")):
        rows = n if nodes is None else nodes.shape[0]
        for self_loop in (False, True):
            buf = torch.full((rows + 1, dim + pad), SENTINEL_BITS, dtype=torch.int32, device="cuda")
            out = ops.csr_mean(rp, cl, table, nodes=nodes, self_loop=self_loop, any_nonempty=flag, out=buf.view(torch.float32)[:rows, :dim])
            assert out.data_ptr() == buf.data_ptr()
            assert bool((buf[:rows, dim:] == SENTINEL_BITS).all()), "columns [dim, ldo) written"
            assert bool((buf[rows] == SENTINEL_BITS).all()), "the row past n written"
            assert not bool((buf[:rows, :dim] == SENTINEL_BITS).any()), "an element of out[:n, :dim] was not stored"
            assert bits_equal(out, ops.csr_mean(rp, cl, table, nodes=nodes, self_loop=self_loop, any_nonempty=flag)), "ldo changes the bits"


@pytest.mark.parametrize("self_loop", [False, True])
def test_csr_mean_node_ids_outside_the_graph_are_empty_rows(self_loop):
    num_nodes, dim = 40, 4
    rowptr, col = _small_csr(num_nodes, 5, seed=1)
    table = np.random.default_rng(2).standard_normal((num_nodes, dim)).astype(np.float32)
    g = Guarded(rowptr, col, table)
    ids = np.array([3, -1, 5, -G, num_nodes, 7, num_nodes + G - 1, 0], dtype=np.int32)
    outside = (ids < 0) | (ids >= num_nodes)
    nodes = torch.from_numpy(ids).cuda()
    inside = ids[~outside].astype(np.int64)
    for flag, fill_nan in ((_flag(1), True), (_flag(0), False), (None, False)):
        out = g.mean(nodes=nodes, self_loop=self_loop, flag=flag).cpu().numpy()
        rows = out[outside]
        assert np.isnan(rows).all() if fill_nan else not rows.any(), "a node id outside [0, num_nodes) is an empty row without a self term"
        ref, bar, ceff = csr_rows_reference(rowptr, col, table, nodes=inside, self_loop=self_loop, flag=fill_nan)
        assert ceff[-1] == (1 if self_loop else 0)                      # node 0: an empty row INSIDE the graph has a self term
        miss = plan_miss(out[~outside], ref, bar, f"rows inside the graph, self_loop={self_loop}")
        assert miss is None, miss


@pytest.mark.parametrize("self_loop", [False, True])
def test_csr_mean_clamps_neighbour_ids_into_the_table(self_loop):
    """table_rows < num_nodes through the C entry: ids below 0 and at or above table_rows read rows 0 and table_rows - 1, bit for
    bit the call on np.clip(col); the count is still the degree.  "Row v holds v" is decided on the ids as stored -- row 29 holds 33,
    which reads row 29 but is not node 29, so the self term joins -- and the self row of a node past the table is the last row."""
    table_rows, num_nodes, dim = 30, 34, 4
    last = table_rows - 1
    rng = np.random.default_rng(3)
    rowptr, col = _small_csr(num_nodes, 6, seed=4)
    col = rng.integers(-G, table_rows + G, len(col)).astype(np.int32)
    assert rowptr[last + 1] > rowptr[last]
    col[rowptr[last]:rowptr[last + 1]][col[rowptr[last]:rowptr[last + 1]] == last] = 2
    col[rowptr[last]] = num_nodes - 1
    assert (col < 0).any() and (col >= num_nodes).any() and ((col >= table_rows) & (col < num_nodes)).any()
    table = rng.standard_normal((table_rows, dim)).astype(np.float32)
    clipped = np.clip(col, 0, last)
    deg = np.diff(rowptr)
    own = np.array([(col[rowptr[v]:rowptr[v + 1]] == v).any() for v in range(num_nodes)])
    own_clipped = np.array([(clipped[rowptr[v]:rowptr[v + 1]] == v).any() for v in range(num_nodes)])
    assert own_clipped[last] and not own[last] and not own[num_nodes - 2:].any()
    ref, bar = np.zeros((num_nodes, dim)), np.zeros((num_nodes, dim))
    for v in range(num_nodes):                                          # fp64 from the written rule, the self row clamped too
        rows = table.astype(np.float64)[clipped[rowptr[v]:rowptr[v + 1]]]
        if self_loop and not own[v]:
            rows = np.concatenate([rows, table.astype(np.float64)[min(v, last)][None]])
        if len(rows):
            ref[v], bar[v] = rows.mean(0), plan_gamma(deg[v], 2) * np.abs(rows).sum(0) / len(rows)
        else:
            ref[v] = np.nan
    for max_edges in (None, 0):
        got = Guarded(rowptr, col, table).mean(self_loop=self_loop, flag=_flag(1), max_edges=max_edges)
        want = Guarded(rowptr, clipped, table).mean(self_loop=self_loop, flag=_flag(1), max_edges=max_edges)
        same = torch.from_numpy((own == own_clipped) | (not self_loop)).cuda()
        assert bits_equal(got[same], want[same]), "out-of-range ids are not read as the clipped ids"
        miss = plan_miss(got.cpu().numpy(), ref, bar, f"clamped neighbour ids, self_loop={self_loop}")
        assert miss is None, miss


def test_csr_mean_clamps_row_pointers_and_makes_them_non_decreasing():
    """A numpy mirror of row_span: b = min(max(rowptr[v], 0), total), e = min(max(rowptr[v + 1], b), total), total =
    rowptr[num_nodes].  The result is that of the clean CSR whose row v is col[b:e]."""
    num_nodes, dim = 14, 4
    rowptr, col = _small_csr(num_nodes, 2, seed=5, long_deg=2 * E + 1)
    total = int(rowptr[-1])
    bad = rowptr.copy()
    bad[0] = -3                                                         # negative
    bad[5] = bad[4] - 2                                                 # decreasing: row 4 is empty, row 5 starts two entries early
    bad[9] = total + G - 1                                              # above the total: row 8 runs to the end, row 9 is empty
    bad[3] = rowptr[3] - G + 1                                          # the long row 2 loses entries, row 3 gains them
    assert bad[-1] == total and (np.diff(bad) < 0).any() and bad.min() >= -G and bad.max() < total + G
    b = np.minimum(np.maximum(bad[:-1], 0), total)
    e = np.minimum(np.maximum(bad[1:], b), total)
    clean_rp = np.zeros(num_nodes + 1, dtype=np.int64)
    np.cumsum(e - b, out=clean_rp[1:])
    clean_col = np.concatenate([col[lo:hi] for lo, hi in zip(b, e)])
    assert (e - b)[4] == 0 and (e - b)[9] == 0 and e[8] == total and (e - b)[2] > E and clean_rp[-1] != total
    table = np.random.default_rng(6).standard_normal((num_nodes, dim)).astype(np.float32)
    for self_loop in (False, True):
        for max_edges in (None, 0):
            got = Guarded(bad, col, table).mean(self_loop=self_loop, flag=_flag(1), max_edges=max_edges)
            want = Guarded(clean_rp, clean_col, table).mean(self_loop=self_loop, flag=_flag(1), max_edges=max_edges)
            assert bits_equal(got, want), (self_loop, max_edges)
        ref, bar, _ = csr_rows_reference(clean_rp, clean_col, table, self_loop=self_loop, flag=True)
        miss = plan_miss(got.cpu().numpy(), ref, bar, f"clamped row pointers, self_loop={self_loop}")
        assert miss is None, miss


def test_csr_mean_counts_with_multiplicity_and_finds_itself_as_a_set():
    num_nodes, dim = 12, 4
    rows = {v: [] for v in range(num_nodes)}
    rows[1] = [4, 1, 5, 1]                                              # v twice: count 4, no self term
    rows[2] = [7, 7, 7, 3]                                              # another id three times: count 4 (+ the self term)
    rows[6] = [int(x) for x in np.random.default_rng(7).choice([0, 3, 4, 5, 8, 9], 2 * E)] + [6]     # v only in the last entry of the last chunk
    rows[10] = [10]
    rowptr = np.concatenate([[0], np.cumsum([len(rows[v]) for v in range(num_nodes)])]).astype(np.int64)
    col = np.concatenate([np.asarray(rows[v], dtype=np.int32) for v in range(num_nodes)])
    table = np.random.default_rng(8).standard_normal((num_nodes, dim)).astype(np.float32)
    g = Guarded(rowptr, col, table)
    for self_loop in (False, True):
        ref, bar, ceff = csr_rows_reference(rowptr, col, table, self_loop=self_loop, flag=True)
        assert [int(ceff[v]) for v in (1, 2, 6, 10, 0)] == [4, 4 + self_loop, 2 * E + 1, 1, int(self_loop)]
        got = g.mean(self_loop=self_loop, flag=_flag(1))
        miss = plan_miss(got.cpu().numpy(), ref, bar, f"multiplicity, self_loop={self_loop}")
        assert miss is None, miss
        assert bits_equal(got, g.mean(self_loop=self_loop, flag=_flag(1), max_edges=0))


def test_csr_mean_flag_zero_in_a_batch_with_edges_and_a_misaligned_table():
    num_nodes, dim, ld = 40, 8, 12
    rowptr, col = _small_csr(num_nodes, 5, seed=9)
    table = np.random.default_rng(10).standard_normal((num_nodes, dim)).astype(np.float32)
    ref, bar, ceff = csr_rows_reference(rowptr, col, table, flag=False)
    assert (ceff == 0).sum() >= 2
    aligned = Guarded(rowptr, col, table, ld=ld)
    got = aligned.mean(flag=_flag(0))
    assert not got.cpu().numpy()[ceff == 0].any(), "flag 0: the empty rows of a batch that has edges are zeros"
    miss = plan_miss(got.cpu().numpy(), ref, bar, "flag 0")
    assert miss is None, miss
    # the table 4 bytes off a 16-byte boundary, a width divisible by 4: the 4-byte kernel, the same arithmetic
    flat = torch.full((1 + (num_nodes + 2 * G) * ld,), 1e30, device="cuda")
    off = flat[1:].view(num_nodes + 2 * G, ld)
    off[G:G + num_nodes, :dim] = torch.from_numpy(table).cuda()
    shifted = Guarded(rowptr, col, table, ld=ld)
    shifted._keep += (flat,)
    shifted.table = off[G:G + num_nodes, :dim]
    assert shifted.table.data_ptr() % 16 == 4 and aligned.table.data_ptr() % 16 == 0
    for self_loop in (False, True):
        got = shifted.mean(self_loop=self_loop, flag=_flag(1))
        ref, bar, _ = csr_rows_reference(rowptr, col, table, self_loop=self_loop, flag=True)
        miss = plan_miss(got.cpu().numpy(), ref, bar, f"misaligned table, self_loop={self_loop}")
        assert miss is None, miss
        assert bits_equal(got, aligned.mean(self_loop=self_loop, flag=_flag(1)))
