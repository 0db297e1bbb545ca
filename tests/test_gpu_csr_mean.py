"""sage_csr_mean (full-neighbourhood mean straight from the CSR, aggregators.py:47-48 num_sample=None) on the MI355X:
against fp64 row sums computed by torch on the CPU, the reference's NaN / zero rule, and bitwise reproducibility."""
import numpy as np
import pytest
import torch

from sage355 import native, ops
from sage355.graph import rmat_graph
from sage355.inference import _nonempty_flag
from util import assert_close_rowmax, load_golden

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
    for self_loop in (False, True):
        full = ops.csr_mean(rp, cl, table, self_loop=self_loop, any_nonempty=flag)
        exp_rows = np.concatenate([np.arange(40), [7, 8, 9]])
        assert_close_rowmax(full.cpu()[exp_rows], fp64_mean(rowptr, col, table64, exp_rows, self_loop, True),
                            what=f"all rows dim={dim} ld={dim + pad} self_loop={self_loop}")
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
