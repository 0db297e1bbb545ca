"""The CSR chunk planner (csrc/sage_csr_common.h: count -> carry -> expand, chunk_item, chunked_row_sum) on the MI355X, driven past one
thread, wave, block and carry pass through every entry point that plans rows.

The cases (tests/util.py, shared with tests/test_csr_plan_host.py): "small", 3 * 2048 + 5 rows with a long row (513, 1024, 1025, 1537
entries: 2, 2, 3, 4 chunks) on either side of every seam of the count scan; "big", 1025 * 2048 + 3 rows (1026 count blocks: the carry
kernel's second pass) with long rows in block 0, at the last row the first pass covers, the first of the second pass and the last row.
Every output is compared whole, every row, with fp64 (np.add.reduceat / np.add.at) under a derived per-element bar (Higham's gamma_m
times the sum of the terms' magnitudes, util.plan_gamma), and bit for bit with the same call at max_edges = 0, whose long rows are
summed in place without the item offsets.  The plan itself -- off[] and carry[nb] in the workspace -- is read back after sage_csr_mean
and compared with the numpy planner: that is what sees a planner that sends every hub to the fall-back, which changes no bit.
Every workspace carries a 256-byte tail of 0xA5 that must survive the call."""
import time

import numpy as np
import pytest
import torch

from sage355 import ops
from util import (PLAN_CARRY, PLAN_CHUNK, PLAN_LONG_BIG, PLAN_LONG_SMALL, PLAN_N_BIG, PLAN_N_SMALL, PLAN_TILE, csr_plan_case,
                  csr_plan_perm, csr_plan_reference, csr_rows_reference, embed_plan_case, embed_plan_reference, plan_gamma,
                  plan_item_cap, plan_miss, plan_tight_max_edges)

pytestmark = pytest.mark.gpu
DEV = "cuda"
TAIL = 256


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def guarded(need):
    """A workspace of `need` bytes and a tail: (the whole allocation, the part the call is given)"""
    ws = torch.full((need + TAIL,), 0xA5, dtype=torch.uint8, device=DEV)
    return ws, ws[:need]


def tail_intact(ws):
    return bool((ws[-TAIL:] == 0xA5).all())


class Case:
    """One planner case on the host and the device, with what the tests share: tables, the node list, the forward graph whose
    TRANSPOSE is the case (so that the backward's long rows sit at the case's positions)."""

    def __init__(self, name):
        self.small = name == "small"
        self.n, self.long_rows = (PLAN_N_SMALL, PLAN_LONG_SMALL) if self.small else (PLAN_N_BIG, PLAN_LONG_BIG)
        self.rowptr, self.col, self.deg = csr_plan_case(self.n, self.long_rows, seed=1 if self.small else 2, filler=6 if self.small else 1)
        self.perm = csr_plan_perm(self.n, self.long_rows, seed=3)
        assert np.array_equal(np.nonzero(self.deg[self.perm] > PLAN_CHUNK)[0], self.long_rows)
        self.rp_d, self.col_d = dev(self.rowptr), dev(self.col)
        self.perm_d = dev(self.perm.astype(np.int32))
        self.flag = torch.ones(1, dtype=torch.int32, device=DEV)
        self._tables, self._fwd = {}, None

    def table(self, dim):
        if dim not in self._tables:
            t = np.random.default_rng(100 + dim).standard_normal((self.n, dim)).astype(np.float32)
            self._tables[dim] = (t, dev(t))
        return self._tables[dim]

    def forward_graph(self):
        """(rowptr_f, col_f) on the host whose transpose has the case's row lengths, and that transpose as ops.csr_transpose builds it"""
        if self._fwd is None:
            rp_f, col_f = ops.csr_transpose(torch.from_numpy(self.rowptr), torch.from_numpy(self.col))
            rp_t, col_t = ops.csr_transpose(rp_f, col_f)
            assert np.array_equal(np.diff(rp_t.numpy()), self.deg)
            self._fwd = (rp_f, col_f, rp_t, col_t)
        return self._fwd


_cases = {}


@pytest.fixture(scope="module", autouse=True)
def drop_the_cases_afterwards():
    yield
    _cases.clear()
    torch.cuda.empty_cache()


def case_of(name):
    if name not in _cases:
        _cases[name] = Case(name)
    return _cases[name]


def read_plan(ws, n):
    """off[0 .. n) and carry[0 .. nb] of a workspace after a call: chunk_ws's first two pieces, each on a 256-byte boundary"""
    nb = -(-n // PLAN_TILE)
    at = (n * 8 + 255) // 256 * 256
    return ws[:n * 8].view(torch.int64).cpu().numpy(), ws[at:at + (nb + 1) * 8].view(torch.int64).cpu().numpy()


def mean_call(c, dim, self_loop, nodes, max_edges=None, **kw):
    """ops.csr_mean on a guarded workspace -> (out, the workspace)"""
    n = c.n if nodes is None else nodes.shape[0]
    me = len(c.col) if max_edges is None else max_edges
    ws, part = guarded(ops.csr_mean_workspace_bytes(n, me, dim))
    table = kw.pop("table", None)
    out = ops.csr_mean(c.rp_d, c.col_d, c.table(dim)[1] if table is None else table, nodes=nodes, self_loop=self_loop, any_nonempty=c.flag,
                       max_edges=me, workspace=part, **kw)
    assert tail_intact(ws), "csr_mean wrote past its workspace"
    return out, ws


def check_plan(ws, deg, what):
    """The white-box check: off[r] of every row and carry[nb] against the numpy planner"""
    _, off, total = csr_plan_reference(deg)
    got_off, got_carry = read_plan(ws, len(deg))
    long_rows = np.nonzero(deg > PLAN_CHUNK)[0]
    assert got_carry[-1] == total, f"{what}: carry[nb] = {got_carry[-1]}, the plan has {total} items"
    assert np.array_equal(got_off[long_rows], off[long_rows]), \
        f"{what}: first items of the long rows {got_off[long_rows].tolist()}, expected {off[long_rows].tolist()}"
    assert np.array_equal(got_off, off), f"{what}: off[] is not the exclusive prefix sum of the rows' chunk counts"


def mean_checks(c, dim, self_loop, form):
    nodes_h, nodes_d = (None, None) if form == "all" else (c.perm, c.perm_d)
    what = f"csr_mean {'small' if c.small else 'big'} dim {dim} self_loop {self_loop} {form}"
    out, ws = mean_call(c, dim, self_loop, nodes_d)
    ref, bar, _ = csr_rows_reference(c.rowptr, c.col, c.table(dim)[0], nodes=nodes_h, self_loop=self_loop, flag=True)
    miss = plan_miss(out.cpu().numpy(), ref, bar, what)
    assert miss is None, miss
    deg = c.deg if nodes_h is None else c.deg[nodes_h]
    check_plan(ws, deg, what)
    in_place, _ = mean_call(c, dim, self_loop, nodes_d, max_edges=0)
    assert bits_equal(out, in_place), f"{what}: the chunk pass and the rows summed in place differ"
    # an item list exactly as long as the plan: a row whose offset were too large by anything would fall back (and change no bit)
    total = int(csr_plan_reference(deg)[2])
    tight = plan_tight_max_edges(len(deg), total)
    assert total <= plan_item_cap(len(deg), tight) < total + 2
    out_t, ws_t = mean_call(c, dim, self_loop, nodes_d, max_edges=tight)
    check_plan(ws_t, deg, what + " (tight item list)")
    assert bits_equal(out, out_t)
    return out


# ---------------------------------------------------------------------------------------------------------------- the small case
@pytest.mark.parametrize("form", ["all", "nodes"])
@pytest.mark.parametrize("self_loop", [False, True])
@pytest.mark.parametrize("dim", [4, 3])
def test_csr_mean_small(dim, self_loop, form):
    mean_checks(case_of("small"), dim, self_loop, form)


def test_csr_mean_nodes_is_not_the_full_result_by_accident():
    c = case_of("small")
    assert not np.any(c.perm[list(c.long_rows)] == np.asarray(c.long_rows))
    full, _ = mean_call(c, 4, True, None)
    sub, _ = mean_call(c, 4, True, c.perm_d)
    assert bits_equal(sub, full[c.perm_d.long()])
    assert not bits_equal(sub, full)


@pytest.mark.parametrize("self_loop", [False, True])
def test_csr_mean_indexed_small(self_loop):
    """index = a permutation: the bits of the call on the materialised table embed[index], which is itself checked against fp64"""
    c = case_of("small")
    embed_h, embed_d = c.table(4)
    index = np.random.default_rng(9).permutation(c.n)
    mat = embed_d[dev(index)]
    got, _ = mean_call(c, 4, self_loop, None, index=dev(index.astype(np.int32)))
    want, _ = mean_call(c, 4, self_loop, None, table=mat)
    assert bits_equal(got, want)
    in_place, _ = mean_call(c, 4, self_loop, None, index=dev(index.astype(np.int32)), max_edges=0)
    assert bits_equal(got, in_place)
    ref, bar, _ = csr_rows_reference(c.rowptr, c.col, embed_h[index], self_loop=self_loop, flag=True)
    miss = plan_miss(got.cpu().numpy(), ref, bar, f"csr_mean indexed small self_loop {self_loop}")
    assert miss is None, miss


def sum_checks(c, dim):
    what = f"csr_sum {'small' if c.small else 'big'} dim {dim}"
    outs = []
    for me in (len(c.col), 0):
        ws, part = guarded(ops.csr_sum_workspace_bytes(c.n, me, dim))
        outs.append(ops.csr_sum(c.rp_d, c.col_d, c.table(dim)[1], max_edges=me, workspace=part))
        assert tail_intact(ws), "csr_sum wrote past its workspace"
    ref, bar, _ = csr_rows_reference(c.rowptr, c.col, c.table(dim)[0], mean=False)
    miss = plan_miss(outs[0].cpu().numpy(), ref, bar, what)
    assert miss is None, miss
    assert bits_equal(outs[0], outs[1]), f"{what}: the chunk pass and the rows summed in place differ"


@pytest.mark.parametrize("dim", [4, 3])
def test_csr_sum_small(dim):
    sum_checks(case_of("small"), dim)


def backward_reference(c, g, self_loop):
    """fp64 adjoint of csr_mean over the forward graph, by node: (want, bar, extra).  w_v = 1 / count exactly; row u collects
    w_v g_v over its transposed entries v (np.add.reduceat), and its own term if it joined its own mean."""
    rp_f, col_f, rp_t, col_t = (x.numpy() for x in c.forward_graph())
    n = c.n
    deg_f = np.diff(rp_f)
    src = np.repeat(np.arange(n), deg_f)
    own = np.zeros(n, dtype=bool)
    own[src[col_f == src]] = True
    extra = ~own if self_loop else np.zeros(n, dtype=bool)
    cnt = deg_f + extra
    w = np.where(cnt > 0, 1.0 / np.maximum(cnt, 1), 0.0)
    term = g.astype(np.float64) * w[:, None]
    want, mass = np.zeros_like(term), np.zeros_like(term)
    has = c.deg > 0
    rows = term[col_t]
    want[has] = np.add.reduceat(rows, rp_t[:-1][has], axis=0)
    mass[has] = np.add.reduceat(np.abs(rows), rp_t[:-1][has], axis=0)
    want[extra] += term[extra]
    mass[extra] += np.abs(term[extra])
    return want, plan_gamma(c.deg + extra, 2)[:, None] * mass, extra


def backward_checks(c, dim, self_loop, grouped):
    what = f"csr_mean_backward{'_grouped' if grouped else ''} {'small' if c.small else 'big'} dim {dim} self_loop {self_loop}"
    rp_f, col_f, rp_t, col_t = c.forward_graph()
    g = np.random.default_rng(200 + dim).standard_normal((c.n, dim)).astype(np.float32)
    g_d = dev(g)
    want, bar, _ = backward_reference(c, g, self_loop)
    outs = []
    if grouped:
        index = torch.from_numpy(c.perm)                            # node u's row is embed[perm[u]]: long nodes keep long positions
        gt = ops.csr_transpose_grouped(rp_f, col_f, index, c.n, self_loop=self_loop)
        assert np.array_equal(np.nonzero(np.diff(gt.rowptr.numpy()) > PLAN_CHUNK)[0], c.long_rows)
        gt_d = ops.GroupedTranspose(gt.rowptr.to(DEV), gt.col.to(DEV), gt.self_loop)
        by_row, bar_row = np.zeros_like(want), np.zeros_like(bar)
        by_row[c.perm], bar_row[c.perm] = want, bar
        want, bar = by_row, bar_row
        for me in (gt.col.numel(), 0):
            ws, part = guarded(ops.csr_mean_backward_grouped_workspace_bytes(c.n, c.n, me, dim))
            outs.append(ops.csr_mean_backward_grouped(rp_f.to(DEV), col_f.to(DEV), gt_d, g_d, max_edges=me, workspace=part))
            assert tail_intact(ws), what + " wrote past its workspace"
    else:
        for me in (len(c.col), 0):
            ws, part = guarded(ops.csr_mean_backward_workspace_bytes(c.n, c.n, me, dim))
            outs.append(ops.csr_mean_backward(rp_f.to(DEV), col_f.to(DEV), rp_t.to(DEV), col_t.to(DEV), g_d, self_loop=self_loop, max_edges=me,
                                              workspace=part))
            assert tail_intact(ws), what + " wrote past its workspace"
    miss = plan_miss(outs[0].cpu().numpy(), want, bar, what)
    assert miss is None, miss
    assert bits_equal(outs[0], outs[1]), f"{what}: the chunk pass and the rows summed in place differ"


@pytest.mark.parametrize("grouped", [False, True])
@pytest.mark.parametrize("self_loop", [False, True])
@pytest.mark.parametrize("dim", [4, 3])
def test_csr_mean_backward_small(dim, self_loop, grouped):
    backward_checks(case_of("small"), dim, self_loop, grouped)


def frontier_checks(c):
    """Seeds = the case's rows (a node list that keeps the long rows in place, some short seeds twice) over a graph in which every
    entry of a long row names a node of its own and the short rows share theirs: a chunk that nobody walks leaves 512 ids out."""
    n, e = c.n, len(c.col)
    is_long = np.repeat(c.deg > PLAN_CHUNK, c.deg)
    col = np.where(is_long, n + np.arange(e), n + e + c.col.astype(np.int64)).astype(np.int32)
    num_nodes = 2 * n + e
    rowptr = np.concatenate([c.rowptr, np.full(num_nodes - n, e, dtype=np.int64)])
    seeds = c.perm.copy()
    short = np.nonzero(c.deg[c.perm] <= PLAN_CHUNK)[0]
    twice = short[(short % 5 == 0) & np.isin(short - 1, short)]
    seeds[twice] = seeds[twice - 1]
    assert np.array_equal(np.nonzero(c.deg[seeds] > PLAN_CHUNK)[0], c.long_rows)
    uniq = np.unique(seeds)
    member = np.zeros(n, dtype=bool)
    member[uniq] = True
    union = np.unique(np.concatenate([uniq, col[np.repeat(member, c.deg)]]))
    rp_d, col_d, seeds_d = dev(rowptr), dev(col), dev(seeds.astype(np.int32))
    for me in (e, 0):
        fr = ops.CsrFrontier(num_nodes, DEV)
        ws, fr.workspace = guarded(ops.csr_frontier_workspace_bytes(n, me))
        ops.csr_frontier(rp_d, col_d, seeds_d, fr, max_edges=me)
        assert tail_intact(ws), "csr_frontier wrote past its workspace"
        count = fr.size()
        nodes_out, pos = fr.nodes[:count].cpu().numpy(), fr.pos.cpu().numpy()
        assert count == len(union) and np.array_equal(np.sort(nodes_out), union), f"max_edges {me}: the set is not numpy's union, each id once"
        assert np.array_equal(pos[nodes_out], np.arange(count)), "pos[nodes_out[i]] != i"
        assert int((pos != -1).sum()) == count, "pos names a row for an id outside the set"


def test_csr_frontier_small():
    frontier_checks(case_of("small"))


def embed_checks(c):
    what = f"embed_grad {'small' if c.small else 'big'}"
    nbr, cnt = embed_plan_case(c.n, c.long_rows, seed=5)
    g = np.random.default_rng(6).standard_normal((len(cnt), 4)).astype(np.float32)
    ws, part = guarded(ops.embed_grad_workspace_bytes(len(cnt), nbr.shape[1], c.n, 4))
    out = ops.embed_grad(dev(g), dev(nbr), dev(cnt), c.n, workspace=part)
    assert tail_intact(ws), "embed_grad wrote past its workspace"
    ref, bar = embed_plan_reference(g, nbr, cnt, c.n)
    terms = np.bincount(nbr[nbr >= 0], minlength=c.n)
    assert np.array_equal(np.nonzero(terms > PLAN_CHUNK)[0], c.long_rows) and 15_000 <= int(cnt.sum()) <= 17_000
    miss = plan_miss(out.cpu().numpy(), ref, bar, what)
    assert miss is None, miss


def test_embed_grad_small():
    embed_checks(case_of("small"))


# ------------------------------------------------------------------------------------------------------------------ the big case
def timed(fn, *args):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn(*args)
    torch.cuda.synchronize()
    print(f"wall time {time.perf_counter() - t0:.2f} s")


@pytest.mark.parametrize("form", ["all", "nodes"])
def test_csr_mean_big(form):
    timed(mean_checks, case_of("big"), 4, True, form)


def test_csr_sum_big():
    timed(sum_checks, case_of("big"), 4)


def test_csr_mean_backward_big():
    timed(backward_checks, case_of("big"), 4, True, False)


def test_csr_frontier_big():
    timed(frontier_checks, case_of("big"))


def test_embed_grad_big():
    timed(embed_checks, case_of("big"))


# ------------------------------------------------------------- the two private scans that hand csr_carry_kernel more than 1024 sums
def test_embed_grad_rows_past_one_carry_pass():
    """32,800 sets of 64 full lists: 2,099,200 sorted slots, 1025 tiles of run heads.  Nearly every term is a run of one; runs of 513,
    600 and 700 terms sit at run index 5, across the end of the last tile the carry kernel's first pass covers, and last (its head
    and its run index both in the second pass)."""
    n, k, dim, lr = 32_800, 64, 4, 0.05
    slots = n * k
    lens_long = {5: 513, PLAN_CARRY * PLAN_TILE - 300 - 512: 600}
    runs = slots - 512 - 599 - 699
    lens = np.ones(runs, dtype=np.int64)
    for u, m in lens_long.items():
        lens[u] = m
    lens[-1] = 700
    start = np.cumsum(lens) - lens
    assert lens.sum() == slots and -(-slots // PLAN_TILE) == PLAN_CARRY + 1
    u_mid = PLAN_CARRY * PLAN_TILE - 300 - 512
    assert start[u_mid] // PLAN_TILE == PLAN_CARRY - 1 and (start[u_mid] + 599) // PLAN_TILE == PLAN_CARRY and u_mid // PLAN_TILE == PLAN_CARRY - 1
    assert start[-1] // PLAN_TILE == PLAN_CARRY and (runs - 1) // PLAN_TILE == PLAN_CARRY
    ids = np.arange(runs) + np.arange(runs) // 3                    # ascending, with gaps: rows that nobody names
    embed_rows = int(ids[-1]) + 5
    rs = np.random.default_rng(8)
    nbr = np.repeat(ids, lens)[rs.permutation(slots)].reshape(n, k).astype(np.int32)
    cnt = np.full(n, k, dtype=np.int32)
    g = rs.standard_normal((n, dim)).astype(np.float32)
    embed_old = rs.standard_normal((embed_rows, dim)).astype(np.float32)
    embed = dev(embed_old)
    ws, part = guarded(ops.embed_grad_rows_workspace_bytes(n, k, embed_rows, dim))
    t0 = time.perf_counter()
    rows_out, num, grad_rows = ops.embed_grad_rows(dev(g), dev(nbr), dev(cnt), embed_rows, embed=embed, lr=lr, workspace=part)
    assert tail_intact(ws), "embed_grad_rows wrote past its workspace"
    assert int(num.item()) == runs
    assert np.array_equal(rows_out[:runs].cpu().numpy(), ids), "rows_out is not np.unique of the ids, ascending"
    ref, bar = embed_plan_reference(g, nbr, cnt, embed_rows, rows=ids)
    got = grad_rows[:runs].cpu().numpy()
    miss = plan_miss(got, ref, bar, "embed_grad_rows")
    assert miss is None, miss
    # embed[e] = fmaf(-lr, s, embed[e]) on the touched rows: one fp32 rounding of the exact value (the 2^-20 covers the fp64
    # reference's own rounding); every other row keeps its bits
    new = embed.cpu().numpy()
    exact = embed_old[ids].astype(np.float64) - float(np.float32(lr)) * got.astype(np.float64)
    assert np.all(np.abs(new[ids] - exact) <= 2.0 ** -24 * np.abs(exact) * (1 + 2.0 ** -20)), "a touched row is not fma(-lr, sum, row)"
    untouched = np.ones(embed_rows, dtype=bool)
    untouched[ids] = False
    assert untouched.sum() > runs // 4 and np.array_equal(new[untouched].view(np.int32), embed_old[untouched].view(np.int32))
    print(f"wall time {time.perf_counter() - t0:.2f} s")


@pytest.mark.parametrize("self_loop", [False, True])
def test_csr_mean_backward_rows_past_one_carry_pass(self_loop):
    """1025 * 2048 + 3 seed rows over a graph of 1,000 nodes: the scans of the seeds' entry and term counts run 1026 blocks.  Nodes
    0..3 have 513, 1024, 1025 and 1537 entries and are the seeds at the big case's four positions; every other seed names an isolated
    node (one self term with self_loop, none without)."""
    num_nodes, dim = 1000, 4
    rs = np.random.default_rng(13)
    deg = np.zeros(num_nodes, dtype=np.int64)
    deg[:4] = (513, 1024, 1025, 1537)
    rowptr = np.zeros(num_nodes + 1, dtype=np.int64)
    np.cumsum(deg, out=rowptr[1:])
    col = rs.integers(4, num_nodes, int(rowptr[-1])).astype(np.int32)
    n = PLAN_N_BIG
    seeds = rs.integers(4, num_nodes, n).astype(np.int32)
    seeds[list(PLAN_LONG_BIG)] = np.arange(4)
    g = rs.standard_normal((n, dim)).astype(np.float32)
    edges = int(rowptr[-1])
    ws, part = guarded(ops.csr_mean_backward_rows_workspace_bytes(n, edges, num_nodes, dim))
    total_terms = torch.zeros(1, dtype=torch.int64, device=DEV)
    t0 = time.perf_counter()
    out = ops.csr_mean_backward_rows(dev(rowptr), dev(col), dev(seeds), dev(g), self_loop=self_loop, max_edges=edges, workspace=part,
                                     total_terms=total_terms)
    assert tail_intact(ws), "csr_mean_backward_rows wrote past its workspace"
    assert int(total_terms.item()) == edges + (n if self_loop else 0)
    want, mass = np.zeros((num_nodes, dim)), np.zeros((num_nodes, dim))
    terms = np.zeros(num_nodes, dtype=np.int64)
    g64 = g.astype(np.float64)
    for r in PLAN_LONG_BIG:                                          # the four seeds with entries
        v = int(seeds[r])
        ids = col[rowptr[v]:rowptr[v + 1]].astype(np.int64)
        t = g64[r] / (deg[v] + (1 if self_loop else 0))
        np.add.at(want, ids, t[None, :])
        np.add.at(mass, ids, np.abs(t)[None, :])
        np.add.at(terms, ids, 1)
    if self_loop:                                                    # no row holds its own node: every seed adds w g to its node
        w = 1.0 / (deg[seeds] + 1)
        np.add.at(want, seeds, g64 * w[:, None])
        np.add.at(mass, seeds, np.abs(g64) * w[:, None])
        np.add.at(terms, seeds, 1)
    miss = plan_miss(out.cpu().numpy(), want, plan_gamma(terms, 2)[:, None] * mass, f"csr_mean_backward_rows self_loop {self_loop}")
    assert miss is None, miss
    print(f"wall time {time.perf_counter() - t0:.2f} s")
