"""sage_csr_mean_bf16 on the MI355X: the full-neighbourhood mean over a feature table STORED as bf16.  Widening a bf16 value to fp32
is exact, so the oracle is exact too -- the BIT RULE: csr_mean(T16) == csr_mean(T16.float()) bitwise, NaNs included, at every shape
at which the kernel takes another path (vector and scalar loads, ld > dim, a table base that is only 2-byte aligned, rows at the edges
of the in-flight groups and of the wave trip, chunked rows with and without workspace room).  One fp64 check besides, so that the
oracle is not only "the other kernel"."""
import numpy as np
import pytest
import torch

from sage355 import native, ops
from util import assert_close_rowmax

pytestmark = pytest.mark.gpu
E = native.CSR_MEAN_CHUNK


def bits_equal(a, b):
    """Bitwise equality, NaNs included (torch.equal says NaN != NaN)."""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def skewed_graph(seed=0):
    """tests/test_gpu_csr_mean.py's generator: rows of degree 0, 1, E-1, E, E+1, 2E, 2E+1 and one star hub of 20E + 37, among rows of
    0..6 edges; some rows hold their own node (rows 8, 9 in their last chunk, the hub in its middle), neighbour lists unsorted."""
    rng = np.random.default_rng(seed)
    n = 24 * E
    special = {0: 0, 1: 1, 2: E - 1, 3: E, 4: E + 1, 5: 2 * E, 6: 2 * E + 1, 7: 20 * E + 37, 8: E + 1, 9: 2 * E + 1}
    deg = rng.integers(0, 7, n)
    for v, d in special.items():
        deg[v] = d
    rowptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(deg, out=rowptr[1:])
    col = rng.integers(0, n, int(rowptr[-1])).astype(np.int32)
    col[rowptr[7]:rowptr[8]] = rng.permutation(n)[: deg[7]]
    for v in (3, 8, 9, 20, 21, 22):
        if deg[v] > 0:
            col[rowptr[v + 1] - 1] = v
    col[rowptr[7] + 5 * E + 3] = 7
    return rowptr, col


def fp64_mean(rowptr, col, table64, nodes, self_loop, nan_flag):
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


def bf16_pair(n, dim, pad, seed, lead=0):
    """(T16, T32): a bf16 table [n, dim] that is columns [lead, lead + dim) of an [n, lead + dim + pad] array, and its exact fp32
    widening with the SAME leading dimension and column offset (so the fp32 kernel takes the path the same shape gives it)."""
    wide = torch.randn(n, lead + dim + pad, generator=torch.Generator().manual_seed(seed)).cuda().to(torch.bfloat16)
    wide32 = wide.float()
    if lead or pad:
        return wide[:, lead:lead + dim], wide32[:, lead:lead + dim]
    return wide, wide32


@pytest.fixture(scope="module")
def t64(graph):
    """One table for the tests that need no particular width: 64 wide, bf16 / its fp32 widening."""
    return bf16_pair(graph[0].shape[0] - 1, 64, 0, 64)


GRID = [(1, 0), (3, 0), (4, 0), (8, 0), (100, 0), (256, 0), (260, 0), (1433, 0), (256, 4), (256, 3), (50, 3)]


@pytest.mark.parametrize("self_loop", [False, True])
@pytest.mark.parametrize("dim,pad", GRID)
def test_the_bit_rule_over_the_shape_grid(graph, dim, pad, self_loop):
    """(256, 4): ld > dim on the vector path; (256, 3): an odd ld forces the scalar path."""
    _, _, rp, cl = graph
    t16, t32 = bf16_pair(rp.shape[0] - 1, dim, pad, dim)
    assert t16.dtype == torch.bfloat16 and t16.stride(0) == dim + pad == t32.stride(0)
    flag = torch.ones(1, dtype=torch.int32, device="cuda")
    got = ops.csr_mean(rp, cl, t16, self_loop=self_loop, any_nonempty=flag)
    want = ops.csr_mean(rp, cl, t32, self_loop=self_loop, any_nonempty=flag)
    assert got.dtype == torch.float32 and got.shape == (rp.shape[0] - 1, dim)
    assert bool(torch.isnan(want[0]).all()) == (not self_loop)             # row 0 is empty: the flag's NaN, or its own row alone
    assert bits_equal(got, want), f"dim={dim} ld={dim + pad} self_loop={self_loop}: {int((got.view(torch.int32) != want.view(torch.int32)).sum())} elements differ"


@pytest.mark.parametrize("self_loop", [False, True])
def test_the_bit_rule_with_a_table_base_that_is_only_2_byte_aligned(graph, self_loop):
    """wide[:, 1:1 + dim] of an array whose ld is a multiple of 4: every shape condition of the vector path holds, only the base
    address does not -- the scalar path has to take it."""
    _, _, rp, cl = graph
    t16, t32 = bf16_pair(rp.shape[0] - 1, 256, 3, 11, lead=1)
    assert t16.stride(0) % 4 == 0 and t16.data_ptr() % 8 == 2
    assert bits_equal(ops.csr_mean(rp, cl, t16, self_loop=self_loop), ops.csr_mean(rp, cl, t32, self_loop=self_loop))


@pytest.mark.parametrize("dim", [64, 50])
def test_nodes_with_repeats_and_ids_outside_the_graph(graph, dim):
    _, _, rp, cl = graph
    n = rp.shape[0] - 1
    t16, t32 = bf16_pair(n, dim, 0, dim + 1)
    rng = np.random.default_rng(dim)
    ids = np.concatenate([np.arange(10), [7, 7, 5, 0, -1, n], rng.integers(0, n, 200), [21, 9, n, -1]]).astype(np.int64)
    nodes = torch.from_numpy(ids.astype(np.int32)).cuda()
    inside = torch.from_numpy((ids >= 0) & (ids < n)).cuda()
    flag = torch.ones(1, dtype=torch.int32, device="cuda")
    for self_loop in (False, True):
        full = ops.csr_mean(rp, cl, t16, self_loop=self_loop, any_nonempty=flag)
        sub = ops.csr_mean(rp, cl, t16, nodes=nodes, self_loop=self_loop, any_nonempty=flag)
        assert bits_equal(sub, ops.csr_mean(rp, cl, t32, nodes=nodes, self_loop=self_loop, any_nonempty=flag))
        assert bits_equal(sub[inside], full[torch.from_numpy(ids).cuda()[inside]]), "csr_mean(nodes=S) != csr_mean()[S] bitwise"
        assert bool(torch.isnan(sub[~inside]).all()), "an id outside the graph is an empty row without a self term"


def test_a_workspace_bound_below_the_truth_costs_speed_not_bits(graph, t64):
    """max_edges = 0: no room at all, every long row is summed chunk by chunk by its row wave; 3E and 25E: room for some chunks."""
    _, _, rp, cl = graph
    t16, t32 = t64
    want = ops.csr_mean(rp, cl, t32, self_loop=True)
    assert bits_equal(ops.csr_mean(rp, cl, t16, self_loop=True), want)
    for max_edges in (0, 3 * E, 25 * E):
        assert bits_equal(ops.csr_mean(rp, cl, t16, self_loop=True, max_edges=max_edges), want), max_edges


EDGE_DEGREES = (7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129)


@pytest.mark.parametrize("dim", [8, 5])
def test_rows_at_the_edges_of_the_in_flight_groups_and_of_the_wave_trip(dim):
    """Row v has EDGE_DEGREES[v] entries: one short of, exactly and one past a group of rows in flight (8 and 16) and a wave trip (64),
    each also with the row's own node as its LAST entry (rows len(EDGE_DEGREES)..)."""
    deg = np.array(EDGE_DEGREES + EDGE_DEGREES, dtype=np.int64)
    n = 200
    rowptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.concatenate([deg, np.zeros(n - len(deg), dtype=np.int64)]), out=rowptr[1:])
    rng = np.random.default_rng(dim)
    col = rng.integers(len(deg), n, int(rowptr[-1])).astype(np.int32)
    for v in range(len(EDGE_DEGREES), len(deg)):
        col[rowptr[v + 1] - 1] = v
    rp, cl = torch.from_numpy(rowptr).cuda(), torch.from_numpy(col).cuda()
    t16, t32 = bf16_pair(n, dim, 0, 3)
    t64f = t16.cpu().double()
    for self_loop in (False, True):
        got = ops.csr_mean(rp, cl, t16, self_loop=self_loop)
        assert bits_equal(got, ops.csr_mean(rp, cl, t32, self_loop=self_loop))
        rows = np.arange(len(deg))
        assert_close_rowmax(got.cpu()[: len(deg)], fp64_mean(rowptr, col, t64f, rows, self_loop, False), what=f"dim={dim} self_loop={self_loop}")


HW_NAN = 0xFFC0                                  # the NaN the MI355X makes of an invalid operation (Inf - Inf): 0xFFC00000 as fp32
SPECIAL = (0x8000, 0x0001, 0x007F, 0x8001, 0x7F7F, 0xFF7F, 0x7F80, 0xFF80, HW_NAN, 0x0080, 0x0000)
OTHER_NANS = (0x7FC0, 0x7FC1, 0x7FFF)            # 0x7FC0: what float("nan") rounds to


def special_table(n, dim, values, seed):
    """bf16 [n, dim]: ordinary values with 2 % of the elements replaced by `values` (raw bf16 bits), each of them at least once in rows
    40.. of column 0, which the hub reads."""
    rng = np.random.default_rng(seed)
    values = np.array(values, dtype=np.uint16)
    bits = torch.randn(n, dim, generator=torch.Generator().manual_seed(seed)).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16).copy()
    where = rng.random((n, dim)) < 0.02
    bits[where] = values[rng.integers(0, len(values), int(where.sum()))]
    bits[40:40 + len(values), 0] = values
    t16 = torch.from_numpy(bits.view(np.int16)).view(torch.bfloat16).cuda()
    t32 = t16.float()
    assert torch.equal(t32.view(torch.int32), (t16.view(torch.int16).to(torch.int32) << 16)), "torch's widening is bits << 16"
    return t16, t32


@pytest.mark.parametrize("dim", [64, 50])
def test_the_bit_rule_for_special_values(graph, dim):
    """-0.0, bf16 subnormals (the smallest, the largest, a negative one), the smallest normal, the largest finite value of either sign,
    +-Inf and NaN among ordinary values: the widening is exact for each, and the fp32 sums that follow are the same operations on the
    same operands -- NaN results included.  The table's NaN is the one the hardware itself makes of an invalid operation (the columns
    hold +Inf and -Inf, so it arises here as well): every NaN of the result then has one bit pattern whatever met whatever.  NaNs of
    other payloads: the next test."""
    _, _, rp, cl = graph
    t16, t32 = special_table(rp.shape[0] - 1, dim, SPECIAL, dim)
    for self_loop in (False, True):
        got = ops.csr_mean(rp, cl, t16, self_loop=self_loop)
        want = ops.csr_mean(rp, cl, t32, self_loop=self_loop)
        assert bool(torch.isnan(want).any()) and bool(torch.isinf(want).any()) and bool(torch.isfinite(want).any())
        assert bits_equal(got, want)


@pytest.mark.parametrize("dim", [64, 50])
def test_nans_of_several_payloads_stay_nans_and_disturb_nothing_else(graph, dim):
    """NaNs of other payloads in the table as well, float("nan")'s 0x7FC0 among them.  Where two DIFFERENT NaNs meet in one addition
    (a partial sum that is the table's NaN and one that is the hardware's Inf - Inf NaN, say), which of the two the result carries
    depends on which operand the compiler put first: an addition commutes, and two compilations of the same sum -- the fp32 kernel
    with 8 rows in flight, the bf16 one with 16 -- need not agree on it.  Seen on the MI355X: with 0x7FC0 as the table's only NaN, 4 of
    786,432 results (width 64, the rows of 513, 513, 1025 and 10,277 entries) were 0x7FC00000 from the bf16 table and 0xFFC00000
    from the fp32 one; no other element differed, with any mix of the special values.  So what is held here is what arithmetic
    defines: the same elements are NaN, and every other element has the same bits."""
    _, _, rp, cl = graph
    t16, t32 = special_table(rp.shape[0] - 1, dim, SPECIAL + OTHER_NANS, dim + 1)
    for self_loop in (False, True):
        got = ops.csr_mean(rp, cl, t16, self_loop=self_loop)
        want = ops.csr_mean(rp, cl, t32, self_loop=self_loop)
        nan = torch.isnan(want)
        assert torch.equal(torch.isnan(got), nan) and bool(nan.any())
        assert bits_equal(torch.where(nan, 0.0, got), torch.where(nan, 0.0, want))
        print(f"dim={dim} self_loop={self_loop}: {int(nan.sum())} NaN results, {int((got.view(torch.int32) != want.view(torch.int32)).sum())} with another payload")


def test_empty_rows_are_zeros_without_the_flag_and_nan_with_it(graph, t64):
    rowptr, _, rp, cl = graph
    t16, _ = t64
    empty = torch.from_numpy(np.nonzero(np.diff(rowptr) == 0)[0]).cuda()
    assert empty.numel() > 100 and int(empty[0]) == 0
    for flag, rule in ((None, "zeros"), (torch.zeros(1, dtype=torch.int32, device="cuda"), "zeros"),
                       (torch.ones(1, dtype=torch.int32, device="cuda"), "nan")):
        out = ops.csr_mean(rp, cl, t16, any_nonempty=flag)
        rows = out[empty]
        assert bool(torch.isnan(rows).all()) if rule == "nan" else bool((rows.view(torch.int32) == 0).all()), rule
        assert not bool(torch.isnan(out[7]).any())
        # with the self term no row is empty
        assert not bool(torch.isnan(ops.csr_mean(rp, cl, t16, self_loop=True, any_nonempty=flag)).any())


def test_two_runs_give_the_same_bits(graph, t64):
    _, _, rp, cl = graph
    t16, _ = t64
    a = ops.csr_mean(rp, cl, t16, self_loop=True)
    b = ops.csr_mean(rp, cl, t16, self_loop=True)
    assert bits_equal(a, b)


@pytest.mark.parametrize("dim,pad", [(256, 0), (50, 3)])
def test_against_the_fp64_mean_of_the_widened_table(graph, dim, pad):
    rowptr, col, rp, cl = graph
    t16, _ = bf16_pair(rowptr.shape[0] - 1, dim, pad, dim)
    table64 = t16.cpu().double()
    rows = np.concatenate([np.arange(40), [7, 8, 9]])
    flag = torch.ones(1, dtype=torch.int32, device="cuda")
    for self_loop in (False, True):
        got = ops.csr_mean(rp, cl, t16, self_loop=self_loop, any_nonempty=flag)
        assert_close_rowmax(got.cpu()[rows], fp64_mean(rowptr, col, table64, rows, self_loop, True), what=f"dim={dim} self_loop={self_loop}")


def test_what_is_not_a_bf16_feature_table_is_refused(graph, t64):
    _, _, rp, cl = graph
    t16, t32 = t64
    n = rp.shape[0] - 1
    index = torch.arange(n, dtype=torch.int32, device="cuda")
    with pytest.raises(native.SageError, match="bfloat16"):
        ops.csr_mean(rp, cl, t16, index=index)
    with pytest.raises(native.SageError):
        ops.csr_mean(rp, cl, t16, out=torch.empty(n, 64, dtype=torch.bfloat16, device="cuda"))
    with pytest.raises(native.SageError):
        ops.csr_mean(rp, cl, t16.t().contiguous().t())                     # inner stride != 1
    with pytest.raises(native.SageError):
        ops.csr_mean(rp, cl, t32.half())                                   # fp16 is not a storage format of the table
    w = torch.zeros(8, 64, device="cuda")
    with pytest.raises(native.SageError):
        ops.linear_act(t16, w)                                             # a bf16 agg
    with pytest.raises(native.SageError):
        ops.linear_act(t32, w.to(torch.bfloat16))                          # a bf16 weight
    with pytest.raises(native.SageError):
        ops.linear_act(t32, torch.zeros(8, 128, device="cuda"), self_tab=t16)
